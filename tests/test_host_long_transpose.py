"""``fft_long_conv_transpose`` / ``FFTLongConvTranspose1d`` without a GPU: exports and the C ABI of the phases plan, argument
checks, the route of every case tests/test_gpu_long_transpose.py runs, the geometry of the phases plan from its descriptor
alone, the module's state, and the identity the phases route rests on, restated in numpy."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import fft_conv_pytorch_amd as pkg
from fft_conv_pytorch_amd import FFTLongConvTranspose1d, _native, fft_long_conv_transpose
from fft_conv_pytorch_amd import functional as F_
from tests.route_util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, C64 = torch.float32, torch.complex64

# the forward table of the GPU tests: the smallest rows that leave the hand-off and still reach each edge
#   1  odd batch (a pair with an empty partner), phases of 501 and 500 taps, phases N = 4096 against spread N = 8192
#   2  depthwise, a stride that is no power of two, a crop that moves the phase of output 0
#   3  K < stride: phase 2 has no tap, its samples and the tail are bias alone
#   4  phases N = 64 x 128, a padding that cuts half the row
#   5  four phases of equal length (also in float16 and bfloat16)
#   6  padding > K - 1
#   7  dilation 2: the zero-spread route
CASES = {
    1: Case(3, 4, 6, (3000,), (1001,), s=2, g=2, tr=True, note="case1"),
    2: Case(2, 3, 3, (2500,), (700,), s=3, p=5, op=2, g=3, tr=True, note="case2"),
    3: Case(1, 2, 2, (3000,), (2,), s=3, op=1, tr=True, note="case3"),
    4: Case(2, 2, 2, (6000,), (4001,), s=2, p=2000, op=1, tr=True, note="case4"),
    5: Case(4, 8, 8, (2000,), (512,), s=4, g=8, tr=True, note="case5"),
    6: Case(2, 2, 2, (3000,), (50,), s=2, p=60, tr=True, note="case6"),
    7: Case(2, 2, 4, (2500,), (600,), s=2, op=1, d=2, tr=True, note="case7"),
}
PHASES_CASES = (1, 2, 3, 4, 5, 6)


def route_of(c, dtype=F32, layouts=("ncl", False)):
    return F_._long_transpose_route((c.B, c.cin, c.size[0]), c.wshape, c.s, c.p, c.op, c.d, c.g, dtype, layouts)


def phases_key(c, has_bias=True):
    return (c.B, c.cin, c.cout, c.g, c.size[0], c.k[0], c.s, c.p, c.op, int(has_bias))


def out_len(c):
    return (c.size[0] - 1) * c.s - 2 * c.p + c.d * (c.k[0] - 1) + c.op + 1


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in ("FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ exports and ABI
def test_names_are_exported():
    assert pkg.fft_long_conv_transpose is F_.fft_long_conv_transpose and "fft_long_conv_transpose" in F_.__all__
    assert pkg.FFTLongConvTranspose1d is pkg.nn.FFTLongConvTranspose1d
    assert issubclass(FFTLongConvTranspose1d, torch.nn.ConvTranspose1d)
    from fft_conv_pytorch_amd.autograd import FFTLongConvTransposeFunction
    assert issubclass(FFTLongConvTransposeFunction, torch.autograd.Function)


def test_new_entry_points_only_and_abi_7():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    new = {"fc_long_phases_geometry", "fc_long_phases_plan_create"}
    assert new <= declared and declared == set(_native.EXPORTS)
    assert re.search(r"int fc_long_phases_geometry\(const fc_long_phases_desc\* desc, int64_t info\[8\]\);", header)
    assert re.search(r"int fc_long_phases_plan_create\(const fc_long_phases_desc\* desc, fc_long_plan\*\* out_plan\);", header)
    lib = _native.load_library()
    for name in _native.EXPORTS:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    # nothing that existed changes: the structs, the kind bits and the key lengths of the other long plans
    assert ctypes.sizeof(_native.FcLongDesc) == 80 and ctypes.sizeof(_native.FcLongExt) == 16
    assert ctypes.sizeof(_native.FcLongPhasesDesc) == 80
    assert (_native.LONG_REAL, _native.LONG_COMPLEX, _native.LONG_CONJ_SIGNAL, _native.LONG_CONJ_TAPS) == (0, 1, 2, 4)
    with pytest.raises(ValueError):
        _native.long_desc((1,) * 12)
    with pytest.raises(ValueError):
        _native.phases_desc((1,) * 11)
    assert _native._PLAN_TAGS == {"long": _native.LongPlan, "long_phases": _native.LongPhasesPlan, "long_decim": _native.LongDecimPlan,
                                  "long_wgrad": _native.LongWgradPlan}
    assert issubclass(_native.LongPhasesPlan, _native.LongPlan)


# ------------------------------------------------------------------------------------------------ arguments
def _cpu(c=CASES[1]):
    return torch.zeros(c.B, c.cin, c.size[0]), torch.zeros(c.wshape), torch.zeros(c.cout)


@pytest.mark.parametrize("kw,text", [
    (dict(stride=0), "stride"), (dict(stride=(2, 2)), "stride"), (dict(stride=2.0), "stride"),
    (dict(dilation=0), "dilation"), (dict(padding=-1), "padding"), (dict(padding="same"), "padding"),
    (dict(output_padding=-1), "output_padding"), (dict(output_padding=2), "output_padding"),
    (dict(dilation=3, output_padding=3), "output_padding"),
    (dict(groups=0), "groups"), (dict(groups=3), "channel mismatch"), (dict(padding=5000), "output length"),
    (dict(channels_last=1), "channels_last"),
])
def test_argument_errors_are_value_errors_before_any_device_call(kw, text, monkeypatch):
    monkeypatch.setattr(_native, "load_library", lambda: pytest.fail("the library was asked"))
    x, w, b = _cpu()
    args = dict(stride=2, groups=2)
    args.update(kw)
    with pytest.raises(ValueError, match=text):
        fft_long_conv_transpose(x, w, b, **args)


def test_shape_errors(monkeypatch):
    monkeypatch.setattr(_native, "load_library", lambda: pytest.fail("the library was asked"))
    x, w, b = _cpu()
    with pytest.raises(ValueError, match="bias"):
        fft_long_conv_transpose(x, w, b[:-1], 2, groups=2)
    with pytest.raises(ValueError, match="expects"):
        fft_long_conv_transpose(x[0], w, b, 2, groups=2)
    with pytest.raises(ValueError, match="channel mismatch"):
        fft_long_conv_transpose(x[:, :2], w, b, 2, groups=2)


def test_accepted_spellings_reach_the_device_gate():
    """1-tuples and output_padding < max(stride, dilation) pass the checks; a CPU tensor then gets fft_long_conv's error."""
    x, w, b = _cpu()
    for kw in (dict(stride=(2,), padding=(3,), output_padding=(1,), dilation=(1,)), dict(stride=1, dilation=3, output_padding=2)):
        with pytest.raises(RuntimeError, match="runs on ROCm devices only"):
            fft_long_conv_transpose(x, w, b, groups=2, **kw)
    with pytest.raises(RuntimeError, match="runs on ROCm devices only"):
        FFTLongConvTranspose1d(4, 6, 1001, stride=2, groups=2)(x)


# ------------------------------------------------------------------------------------------------ routes
def test_routes_of_the_gpu_table(monkeypatch):
    for i, c in CASES.items():
        assert route_of(c) == ("phases" if i in PHASES_CASES else "spread"), i
        assert route_of(c, torch.bfloat16) == route_of(c, torch.float16) == route_of(c), i
        # case 8: complex rows and channels-last tensors stay on the spread row
        assert route_of(c, C64) == "spread", i
        assert route_of(c, F32, ("nlc", False)) == route_of(c, F32, ("ncl", True)) == "spread", i
        assert route_of(c, F32, ("copy", False)) == route_of(c), i
    monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    for i, c in CASES.items():
        assert route_of(c) == "spread", i
    monkeypatch.setenv("FFTCONV_LONG_POLY", "1")
    assert route_of(CASES[1]) == "phases"


def test_handoff_and_the_edges_of_the_phases_route():
    # the zero-spread row, Lout + d*(K-1) points, decides the hand-off: 2*999 + 100 + 99 = 2297; complex rows never
    short = Case(2, 2, 2, (1000,), (100,), s=2, tr=True)
    assert route_of(short) == "handoff" and route_of(short, C64) == "spread"
    edge = Case(1, 1, 1, (1500,), (549,), s=2, op=1, tr=True)    # Lout = 2998 + 549 + 1 = 3548, + 548 = 4096
    assert F_._long_transpose_needs(1500, 549, 2, 0, 1, 1)[0] == 4096 and route_of(edge) == "handoff"
    assert F_._long_transpose_needs(1500, 550, 2, 0, 0, 1)[0] == 4097
    assert route_of(Case(1, 1, 1, (1500,), (550,), s=2, tr=True)) == "phases"
    # stride 1 has one phase, which is the spread row itself
    assert route_of(Case(2, 2, 2, (5000,), (1000,), s=1, tr=True)) == "spread"
    assert route_of(Case(2, 2, 2, (5000,), (1000,), s=64, tr=True)) == "phases"
    assert route_of(Case(2, 2, 2, (5000,), (1000,), s=65, tr=True)) == "spread"


def test_a_row_past_the_spread_limit_runs_by_phases_and_past_both_raises(monkeypatch):
    big = Case(1, 1, 1, (5_000_000,), (1_000_000,), s=4, tr=True)
    spread, phases = F_._long_transpose_needs(5_000_000, 1_000_000, 4, 0, 0, 1)
    assert spread > F_.LONG_MAX_POINTS >= phases
    assert route_of(big) == "phases"
    info = _native.phases_geometry(phases_key(big))
    assert info["N1"] * info["N2"] == 1 << 23 and info["out_len"] == out_len(big)
    with pytest.raises(NotImplementedError, match=r"2\^24"):      # the spread plan of the same row
        _native.long_geometry((1, 1, 1, 1, 5_000_000, 1_000_000, 999_999, 999_999, out_len(big), 1, 0, 0, 4, 1, 1))
    monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    with pytest.raises(NotImplementedError, match=str(spread)):
        route_of(big)
    monkeypatch.delenv("FFTCONV_LONG_POLY")
    with pytest.raises(NotImplementedError, match="2\\*\\*24"):
        route_of(Case(1, 1, 1, (20_000_000,), (1000,), s=2, tr=True))
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.phases_geometry((1, 1, 1, 1, 20_000_000, 1000, 2, 0, 0, 0))


# ------------------------------------------------------------------------------------------------ geometry
def _spread_key(c, has_bias=True):
    drop, n, lead, tail = F_._long_spread_args(c.size[0], c.k[0], c.s, c.p, c.op, c.d)
    return (c.B, c.cin, c.cout, c.g, n, c.k[0], lead, tail, out_len(c), 1, int(has_bias), 0, c.s, c.d, 1)


def test_phases_geometry_of_case_1_against_the_spread_plan():
    c = CASES[1]
    ph, sp = _native.phases_geometry(phases_key(c)), _native.long_geometry(_spread_key(c))
    assert (ph["N1"], ph["N2"]) == (64, 64) and (sp["N1"], sp["N2"]) == (64, 128)
    assert ph["out_len"] == sp["out_len"] == out_len(c) == 6999
    # s phases per filter, but a transform of half the points: the same spectrum, a smaller workspace
    assert ph["spectrum_bytes"] == c.s * c.cout * (c.cin // c.g) * 4096 * 8 == sp["spectrum_bytes"]
    assert ph["workspace_bytes"] == ph["slab_pairs"] * (c.cin + c.s * c.cout) * 4096 * 8
    assert sp["workspace_bytes"] == sp["slab_pairs"] * (c.cin + c.cout) * 8192 * 8 and ph["slab_pairs"] == sp["slab_pairs"] == 2


@pytest.mark.parametrize("i", PHASES_CASES)
def test_phases_geometry_of_the_table(i):
    c = CASES[i]
    info = _native.phases_geometry(phases_key(c))
    n = info["N1"] * info["N2"]
    assert info["out_len"] == out_len(c)
    assert info["spectrum_bytes"] == c.s * c.cout * (c.cin // c.g) * n * 8
    assert info["workspace_bytes"] == info["slab_pairs"] * (c.cin + c.s * c.cout) * n * 8
    need = F_._long_transpose_needs(c.size[0], c.k[0], c.s, c.p, c.op, c.d)[1]
    assert n >= need and (n == 4096 or n < 2 * need), (n, need)
    assert n == {1: 4096, 2: 4096, 3: 4096, 4: 64 * 128, 5: 4096, 6: 4096}[i]


@pytest.mark.parametrize("key,text", [
    ((1, 4, 6, 2, 100, 10, 0, 0, 0, 0), "stride"), ((1, 4, 6, 2, 100, 10, 2, -1, 0, 0), "padding"),
    ((1, 4, 6, 2, 100, 10, 2, 0, 2, 0), "output_padding"), ((1, 4, 6, 4, 100, 10, 2, 0, 0, 0), "divisible"),
    ((1, 4, 6, 2, 100, 10, 2, 200, 0, 0), "output length"), ((0, 4, 6, 2, 100, 10, 2, 0, 0, 0), "positive"),
])
def test_phases_geometry_refuses_bad_descriptors(key, text):
    with pytest.raises(ValueError, match=text):
        _native.phases_geometry(key)


def test_phases_geometry_limits():
    with pytest.raises(NotImplementedError, match="4096"):
        _native.phases_geometry((1, 1, 1, 1, 100, 10, 5000, 0, 0, 0))
    with pytest.raises(NotImplementedError, match=r"2\^29"):          # an output row of 640e6 samples
        _native.phases_geometry((1, 1, 1, 1, 5_000_000, 100, 128, 0, 0, 0))


def test_phases_geometry_refuses_a_slab_whose_inverse_grid_exceeds_one_launch(monkeypatch):
    """4096 pairs x 4096 filters x 2 phases at 64 x 64 points: the passes every long plan runs stay inside 2^31 workgroups
    (2^30 for the rows of W2), the phase blocks of the inverse pass, two of them per filter at NC = 2 with 32 column blocks
    each at the least, do not."""
    key = (8192, 4096, 4096, 4096, 3000, 1001, 2, 0, 0, 0)
    assert _native.phases_geometry(key)["slab_pairs"] < 64         # (the default budget keeps the slabs small)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "2000000")
    with pytest.raises(NotImplementedError, match=r"phases .* exceeds the 2\^31 workgroups"):
        _native.phases_geometry(key)
    assert _native.phases_geometry((2048,) + key[1:])["slab_pairs"] == 1024          # a quarter of the batch fits one launch


# ------------------------------------------------------------------------------------------------ the module
def test_module_interchanges_state_with_conv_transpose1d_and_copies():
    torch.manual_seed(0)
    ref = torch.nn.ConvTranspose1d(4, 6, 1001, stride=2, padding=3, output_padding=1, groups=2)
    layer = FFTLongConvTranspose1d(4, 6, 1001, stride=2, padding=3, output_padding=1, groups=2, channels_last=True)
    assert set(layer.state_dict()) == set(ref.state_dict()) == {"weight", "bias"}
    layer.load_state_dict(ref.state_dict())
    back = torch.nn.ConvTranspose1d(4, 6, 1001, stride=2, padding=3, output_padding=1, groups=2)
    back.load_state_dict(layer.state_dict())
    assert torch.equal(back.weight, ref.weight) and torch.equal(back.bias, ref.bias)
    assert (layer.stride, layer.padding, layer.output_padding, layer.dilation, layer.groups) == \
        (ref.stride, ref.padding, ref.output_padding, ref.dilation, ref.groups)
    layer.__dict__["_spectrum_cache"] = ("tag", object())         # transient acceleration state stays behind
    for clone in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert isinstance(clone, FFTLongConvTranspose1d) and "_spectrum_cache" not in clone.__dict__
        assert torch.equal(clone.weight, layer.weight) and clone.channels_last is True
    assert "channels_last=True" in repr(layer)
    with pytest.raises(ValueError, match="channels_last"):
        FFTLongConvTranspose1d(4, 6, 5, channels_last="yes")
    nobias = FFTLongConvTranspose1d(4, 4, 9, stride=3, bias=False, dtype=torch.bfloat16)
    assert nobias.bias is None and nobias.weight.dtype == torch.bfloat16 and tuple(nobias.weight.shape) == (4, 4, 9)


# ------------------------------------------------------------------------------------------------ the identity
def _conv_transpose(x, w, s, p, op):
    L, K = len(x), len(w)
    full = np.zeros((L - 1) * s + K + op)
    for t in range(L):
        full[t * s:t * s + K] += x[t] * w
    return full[p:p + (L - 1) * s - 2 * p + K + op]


def _by_phases(x, w, s, p, op):
    """y[s*t + q - p] = (w_q * x)[t] with w_q[j] = w[q + s*j]: s ordinary convolutions, interleaved; every output once."""
    L, K = len(x), len(w)
    lout = (L - 1) * s - 2 * p + K + op
    y, hits = np.zeros(lout), np.zeros(lout, dtype=int)
    kp = -(-K // s)
    for q in range(s):
        wq = np.zeros(kp)
        taps = w[q::s]                       # shorter phases and phases with no tap at all read as zero
        wq[:len(taps)] = taps
        conv = np.convolve(x, wq)            # t = 0 .. L + kp - 2
        for t in range((lout - 1 + p) // s + 1):
            n = s * t + q - p
            if 0 <= n < lout:
                y[n] += conv[t] if t < len(conv) else 0.0
                hits[n] += 1
    assert (hits == 1).all()
    return y


@pytest.mark.parametrize("L,K,s,p,op", [
    (30, 11, 2, 0, 0), (25, 7, 3, 5, 2), (30, 2, 3, 0, 1), (60, 41, 2, 20, 1), (20, 8, 4, 0, 0), (30, 5, 2, 6, 0),
    (7, 3, 5, 9, 4), (5, 1, 2, 0, 1), (9, 20, 3, 17, 0), (3, 2, 7, 0, 6),
])
def test_interleaved_phase_convolutions_are_the_transposed_convolution(L, K, s, p, op):
    rng = np.random.default_rng(L + K)
    x, w = rng.integers(-8, 9, L).astype(float), rng.integers(-8, 9, K).astype(float)
    want = _conv_transpose(x, w, s, p, op)
    assert np.array_equal(_by_phases(x, w, s, p, op), want)
    ref = torch.nn.functional.conv_transpose1d(torch.tensor(x)[None, None], torch.tensor(w)[None, None], None, s, p, op)
    assert np.array_equal(ref[0, 0].numpy(), want)


def test_spread_row_arguments_cover_every_output():
    """The zero-spread row: what _long_run is asked for reaches every output and reads only samples some output meets."""
    for L, K, s, p, op, d in [(3000, 1001, 2, 0, 0, 1), (3000, 50, 2, 60, 0, 1), (2500, 600, 2, 0, 1, 2), (10, 3, 4, 9, 3, 1),
                              (5, 2, 3, 7, 0, 1), (2, 2, 2, 2, 0, 1)]:
        lout = (L - 1) * s - 2 * p + d * (K - 1) + op + 1
        if lout < 1:
            continue
        drop, n, lead, tail = F_._long_spread_args(L, K, s, p, op, d)
        if n == 0:
            assert all(not (0 <= s * t + d * k - p < lout) for t in range(L) for k in range(K))
            continue
        assert lead >= 0 and tail >= 0 and lead + s * (n - 1) + 1 + tail >= lout + d * (K - 1)
        met = [t for t in range(L) if any(0 <= s * t + d * k - p < lout for k in (0, K - 1))]
        assert drop <= met[0] and met[-1] < drop + n
        assert lead == d * (K - 1) - p + s * drop             # sample `drop` of x sits where the plan looks for it
