"""Planner arithmetic of the float64 long 1-D route (csrc/long_f64.hip, plan kind ``f64_fft_long``): which plans take it,
their factorisation N = N1 x N2, tiles, sizes and knobs -- no GPU needed, an FC_F64 plan makes no device call -- and a
torch-float64 restatement of its three passes against torch's own convolution.

The twiddle w_N^m of the kernels is sincospi(2 m / N) per point, not a table: m / N is exact in float64 for every m < N
<= 2^22, so there are no host tables whose rounding could be checked here."""
import math

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native

F64 = 1
C2 = 16          # bytes of one complex double
TOL64 = 1e-12    # route_util.TOL64: max|got - want| / max|want|
KNOBS = ("FFTCONV_F64_FFT", "FFTCONV_F64_LONG", "FFTCONV_F64_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_ZEROWRAP")
MODES = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _key(B, ci, co, g, L, K, stride=1, pad=0, dil=1, mode=0, transposed=False, out_pad=0, bias=True):
    return (1, B, ci, co, g, (L,), (K,), (stride,), (pad,), (dil,), mode, bias, 0, transposed, (out_pad,), F64)


def _pow2_at_least(v, lo=12, hi=22):
    lg = lo
    while (1 << lg) < v and lg < hi:
        lg += 1
    return lg


def _cob(B, g, cog, N1, N2):
    """The rule of the tiled 1-D float64 plan on the row pass's workgroups: 8, halved (down to 2) while the launch has
    fewer than 256 workgroups, never more than the group's output channels."""
    nr = 1 if N2 >= 256 else 256 // N2
    cob = 8
    while cob > 2 and (B + 1) // 2 * g * -(-cog // cob) * (N1 // nr) < 256:
        cob //= 2
    return min(cob, cog)


def _assert_long(plan, need, B, ci, co, g):
    r = plan.route
    assert r["kind"] == "f64_fft_long", r
    lg = _pow2_at_least(need)
    assert (r["N1"], r["N2"]) == (1 << lg // 2, 1 << (lg - lg // 2)), (r, need)     # the most balanced split, N2 >= N1
    N = r["N1"] * r["N2"]
    assert N >= need and r["ntiles"] == 1
    assert plan.tile == r["N2"]
    assert r["cob"] == _cob(B, g, co // g, r["N1"], r["N2"])
    assert plan.spectrum_bytes == co * (ci // g) * N * C2
    assert plan.workspace_bytes == (B + 1) // 2 * (ci + co) * N * C2              # W1 + W2 of every batch pair
    assert plan.layout[:2] == (r["N1"], r["N2"])
    return r


def test_long_kernel_takes_the_long_route():
    """B2 4->4 L 5000 K 1100: the direct kernel before this route existed."""
    plan = _native.Plan(_key(2, 4, 4, 1, 5000, 1100))
    r = _assert_long(plan, 5000, 2, 4, 4, 1)
    assert (r["N1"], r["N2"]) == (64, 128)
    assert plan.out_spatial == (3901,)


def test_transposed_and_dilated_keys_take_the_long_route():
    plan = _native.Plan(_key(2, 4, 4, 1, 5000, 1100, transposed=True))
    assert plan.out_spatial == (6099,)
    _assert_long(plan, 6099, 2, 4, 4, 1)           # zero padding absorbs the wrap: the output extent is enough
    plan = _native.Plan(_key(2, 4, 4, 1, 5000, 300, dil=4))
    _assert_long(plan, 5000, 2, 4, 4, 1)
    plan = _native.Plan(_key(3, 6, 4, 2, 5000, 1100, stride=3, pad=200, mode=1))
    _assert_long(plan, 5400, 3, 6, 4, 2)           # a padding mode: the whole padded row


def test_k1025_keeps_the_tiled_route_and_its_words():
    plan = _native.Plan(_key(2, 4, 4, 1, 5000, 1025))
    assert plan.route == {"kind": "f64_fft_1d", "T": 2048, "ntiles": 4, "cob": 2}
    assert plan.tile == 2048 and plan.workspace_bytes == 0
    assert plan.spectrum_bytes == 4 * 4 * 2048 * C2


@pytest.mark.parametrize("knob", ["FFTCONV_F64_FFT", "FFTCONV_F64_LONG"])
def test_knobs_keep_the_direct_kernel(knob, monkeypatch):
    monkeypatch.setenv(knob, "0")
    for key in (_key(2, 4, 4, 1, 5000, 1100), _key(2, 4, 4, 1, 5000, 1100, transposed=True)):
        plan = _native.Plan(key)
        assert plan.route == {"kind": "f64_direct"}
        assert plan.tile == 0 and plan.workspace_bytes == 0 and plan.spectrum_bytes == 4 * 4 * 1100 * 8


def test_knob_2_takes_a_short_kernel(monkeypatch):
    assert _native.Plan(_key(2, 4, 4, 1, 5000, 65)).route["kind"] == "f64_fft_1d"
    monkeypatch.setenv("FFTCONV_F64_LONG", "2")
    _assert_long(_native.Plan(_key(2, 4, 4, 1, 5000, 65)), 5000, 2, 4, 4, 1)
    assert _native.Plan(_key(2, 4, 4, 1, 5000, 15)).route["kind"] == "f64_direct"      # fewer than 16 taps
    assert _native.Plan(_key(2, 4, 4, 1, 30, 3)).route["kind"] == "f64_direct"


def test_valid_call_with_a_kernel_as_long_as_the_row_stays_direct(monkeypatch):
    """K = L - 3, 'valid': four outputs per row, the direct kernel's work is tiny and N log N is not."""
    key = _key(2, 4, 4, 1, 5000, 4997)
    assert _native.Plan(key).route == {"kind": "f64_direct"}
    monkeypatch.setenv("FFTCONV_F64_LONG", "2")             # (the same key without the crossover)
    assert _native.Plan(key).route["kind"] == "f64_fft_long"


def test_crossover_is_work_of_the_direct_kernel_per_transformed_point_and_stage():
    """nout * Cin/g * K >= c * ntiles * N * log2 N, monotone in the kept outputs: some padding between 'valid' (direct) and
    'same' (long) is the first to take the long route, and every larger one takes it too."""
    kinds = [_native.Plan(_key(1, 1, 1, 1, 20000, 20000, pad=p)).route["kind"] for p in range(0, 10001, 500)]
    assert kinds[0] == "f64_direct" and kinds[-1] == "f64_fft_long"
    first = kinds.index("f64_fft_long")
    assert all(k == "f64_direct" for k in kinds[:first]) and all(k == "f64_fft_long" for k in kinds[first:])


def test_forced_factorisation_and_tiles(monkeypatch):
    monkeypatch.setenv("FFTCONV_F64_LONG_N", "64x64")
    plan = _native.Plan(_key(2, 4, 4, 1, 10000, 1100))
    Lf = 10000 - 1100 + 1
    assert plan.route == {"kind": "f64_fft_long", "N1": 64, "N2": 64, "ntiles": -(-Lf // 2997), "cob": _cob(2, 1, 4, 64, 64)}
    assert plan.tile == 64
    assert plan.spectrum_bytes == 4 * 4 * 4096 * C2 and plan.workspace_bytes == 8 * 4096 * C2
    monkeypatch.setenv("FFTCONV_F64_LONG_N", "2048x64")     # a forced split need not be balanced, nor N2 >= N1
    r = _native.Plan(_key(2, 4, 4, 1, 10000, 1100)).route
    assert (r["N1"], r["N2"], r["ntiles"]) == (2048, 64, 1)


def test_rows_past_the_largest_transform_run_in_tiles():
    N = 1 << 22
    L, K = 3 * N, 2000
    r = _native.Plan(_key(1, 64, 64, 1, L, K)).route
    assert (r["kind"], r["N1"], r["N2"]) == ("f64_fft_long", 2048, 2048)
    assert r["ntiles"] == -(-(L - K + 1) // (N - K + 1))
    # a kernel that leaves less than half of the largest transform valid keeps the direct kernel
    assert _native.Plan(_key(1, 64, 64, 1, 3 * N, N // 2 + 2)).route == {"kind": "f64_direct"}


@pytest.mark.parametrize("value", ["64", "64x", "x64", "64x64x", "100x64", "64x4096", "32x64", "64*64", "0x0", "-64x64"])
def test_malformed_factorisation_raises(value, monkeypatch):
    monkeypatch.setenv("FFTCONV_F64_LONG_N", value)
    with pytest.raises(ValueError, match="FFTCONV_F64_LONG_N"):
        _native.Plan(_key(2, 4, 4, 1, 5000, 1100))


def test_forced_factorisation_too_small_raises(monkeypatch):
    monkeypatch.setenv("FFTCONV_F64_LONG_N", "64x64")
    with pytest.raises(ValueError, match="fewer than half"):
        _native.Plan(_key(2, 4, 4, 1, 10000, 3000))          # 1097 valid samples of 4096
    _native.Plan(_key(2, 4, 4, 1, 4000, 3000))               # the whole row fits: one transform, nothing to refuse


def test_slabs_under_the_workspace_budget(monkeypatch):
    N = 8192
    pair_bytes = (4 + 4) * N * C2                            # exactly 1 MiB
    for mb, B, pairs in ((1, 6, 1), (2, 6, 2), (2, 7, 2), (100, 7, 4), (1, 1, 1)):
        monkeypatch.setenv("FFTCONV_LONG_WS_MB", str(mb))
        plan = _native.Plan(_key(B, 4, 4, 1, 5000, 1100))
        assert plan.route["kind"] == "f64_fft_long"
        assert plan.workspace_bytes == pairs * pair_bytes, (mb, B)
        assert plan.spectrum_bytes == 4 * 4 * N * C2


# ------------------------------------------------------------------ the three passes, restated in torch float64
def _axis_src(p, size, pad, mode, up):
    """axis_map.hpp axis_src on a tensor of padded positions: (source index, valid)."""
    pos = p - pad
    if up > 1:
        q = torch.div(pos, up, rounding_mode="floor")
        ok = (pos >= 0) & (q * up == pos) & (q < size)
        return q.clamp(0, size - 1), ok
    inside = (pos >= 0) & (pos < size)
    ok = (pos >= -pad) & (pos < size + pad) if mode != "constant" else inside
    if mode == "reflect":
        src = torch.where(pos < 0, -pos, torch.where(pos >= size, 2 * (size - 1) - pos, pos))
    elif mode == "replicate":
        src = pos.clamp(0, size - 1)
    elif mode == "circular":
        src = torch.where(pos < 0, pos + size, torch.where(pos >= size, pos - size, pos))
    else:
        src = pos
    return src.clamp(0, size - 1), ok


def _three_passes(x, w, b, N1, N2, stride=1, padding=0, dilation=1, groups=1, mode="constant", transposed=False,
                  output_padding=0):
    """long_f64.hip in torch: gather, column transforms and twiddle, row transforms / product / inverse, column inverse
    and the stride predicate, per overlap-save tile and batch pair, into an output filled with NaN."""
    B, Cin, L = x.shape
    K = w.shape[-1]
    kd = (K - 1) * dilation + 1
    if transposed:
        Cout = w.shape[1] * groups
        Lf = (L - 1) * stride - 2 * padding + kd - 1 + output_padding + 1
        pad, up, ostride = kd - 1 - padding, stride, 1
    else:
        Cout = w.shape[0]
        Lf = L + 2 * padding - kd + 1
        pad, up, ostride = padding, 1, stride
    Lout = (Lf - 1) // ostride + 1
    Cig, Cog = Cin // groups, Cout // groups
    N = N1 * N2
    V = N - kd + 1
    ntiles = -(-Lf // V)
    n = torch.arange(N)
    k1, n2 = torch.arange(N1).view(N1, 1), torch.arange(N2).view(1, N2)
    tw = torch.polar(torch.ones(N1, N2, dtype=torch.float64), -2 * math.pi * (k1 * n2).double() / N)     # w_N^(n2 k1)

    def cols_fwd(z):                       # (..., N) -> W1 (..., k1, n2)
        return torch.fft.fft(z.reshape(z.shape[:-1] + (N1, N2)), dim=-2) * tw

    # the filter rows: dilated taps, back to front with the channels exchanged for a transposed plan
    pp = kd - 1 - n if transposed else n
    tap = torch.div(pp, dilation, rounding_mode="floor")
    ok = (pp >= 0) & (tap * dilation == pp) & (tap < K)
    h = torch.zeros(Cout, Cig, N, dtype=torch.complex128)
    for go in range(Cout):
        for i in range(Cig):
            wrow = w[(go // Cog) * Cig + i, go % Cog] if transposed else w[go, i]
            h[go, i, ok] = wrow[tap[ok]].to(torch.complex128)
    H = torch.fft.fft(cols_fwd(h), dim=-1).conj() / N           # [o][i][k1][k2]

    y = torch.full((B, Cout, Lout), float("nan"), dtype=torch.float64)
    for tile in range(ntiles):
        src, valid = _axis_src(tile * V + n, L, pad, mode, up)
        rows = torch.where(valid, x[:, :, src], torch.zeros((), dtype=torch.float64))       # (B, Cin, N)
        t0, limit = tile * V, min(V, Lf - tile * V)
        for pr in range((B + 1) // 2):
            b0 = 2 * pr
            has1 = b0 + 1 < B
            z = torch.complex(rows[b0], rows[b0 + 1] if has1 else torch.zeros_like(rows[b0]))
            X = torch.fft.fft(cols_fwd(z), dim=-1)                                       # (Cin, k1, k2)
            Y = torch.einsum("giab,goiab->goab", X.view(groups, Cig, N1, N2), H.view(groups, Cog, Cig, N1, N2))
            W2 = torch.fft.ifft(Y.reshape(Cout, N1, N2), dim=-1) * N2 * tw.conj()
            out = (torch.fft.ifft(W2, dim=-2) * N1).reshape(Cout, N)                     # t = n1 * N2 + n2
            t = torch.arange(limit)
            keep = t[(t0 + t) % ostride == 0]
            idx = (t0 + keep) // ostride
            bias = b.view(-1, 1) if b is not None else 0.0
            y[b0, :, idx] = out.real[:, keep] + bias
            if has1:
                y[b0 + 1, :, idx] = out.imag[:, keep] + bias
    return y, ntiles


def _reference(x, w, b, stride=1, padding=0, dilation=1, groups=1, mode="constant", transposed=False, output_padding=0):
    if transposed:
        return F.conv_transpose1d(x, w, b, stride=stride, padding=padding, output_padding=output_padding, dilation=dilation,
                                  groups=groups)
    if mode == "constant":
        return F.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)
    return F.conv1d(F.pad(x, (padding, padding), mode=mode), w, b, stride=stride, dilation=dilation, groups=groups)


RESTATED = [
    # B, Cin, Cout, L, K, kwargs: two tiles of 64 x 64 points each
    (3, 4, 6, 5000, 1100, dict(groups=2)),
    (2, 2, 2, 4500, 1100, dict(stride=3, padding=300, mode="reflect")),
    (1, 2, 3, 4000, 1100, dict(padding=400, mode="circular")),
    (2, 3, 2, 4400, 1100, dict(padding=200, mode="replicate")),
    (3, 2, 2, 5200, 300, dict(dilation=4, padding=100)),
    (3, 4, 2, 1600, 1100, dict(stride=2, padding=5, output_padding=1, groups=2, transposed=True)),
]


@pytest.mark.parametrize("case", RESTATED, ids=[f"B{c[0]}c{c[1]}-{c[2]}L{c[3]}K{c[4]}" + "".join(f"-{k}{v}" for k, v in c[5].items())
                                                for c in RESTATED])
def test_three_passes_restated_match_torch(case, monkeypatch):
    B, ci, co, L, K, kw = case
    g = kw.get("groups", 1)
    gen = torch.Generator().manual_seed(B * 1000 + L + K)
    x = torch.randn(B, ci, L, generator=gen, dtype=torch.float64)
    wshape = (ci, co // g, K) if kw.get("transposed") else (co, ci // g, K)
    w = torch.randn(*wshape, generator=gen, dtype=torch.float64)
    b = torch.randn(co, generator=gen, dtype=torch.float64)
    got, ntiles = _three_passes(x, w, b, 64, 64, **kw)
    assert ntiles == 2
    want = _reference(x, w, b, **kw)
    assert got.shape == want.shape
    assert torch.isfinite(got).all(), "a kept sample was never written"
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err < TOL64, err
    # the plan of the same call has the tiles of the restatement
    monkeypatch.setenv("FFTCONV_F64_LONG_N", "64x64")
    monkeypatch.setenv("FFTCONV_F64_LONG", "2")
    plan = _native.Plan(_key(B, ci, co, g, L, K, kw.get("stride", 1), kw.get("padding", 0), kw.get("dilation", 1),
                             MODES[kw.get("mode", "constant")], kw.get("transposed", False), kw.get("output_padding", 0)))
    assert plan.route["kind"] == "f64_fft_long" and plan.route["ntiles"] == 2
    assert plan.out_spatial == (want.shape[-1],)
