"""Planner arithmetic of float64 2-D / 3-D and transposed plans (no GPU needed: an FC_F64 plan makes no device call).
Past the crossover these plans take the FFT path (csrc/nd_f64.hip, 1-D transposed: csrc/fft_f64.hip) and report its
transform lengths, kernel-spectrum and workspace bytes; the direct kernel keeps the rest."""
import pytest

from fft_conv_pytorch_amd import _native

F64 = 1
C2 = 16          # bytes of one complex double


def _key(B, ci, co, g, S, k, stride=None, pad=None, dil=None, mode=0, transposed=False, out_pad=None):
    n = len(S)
    return (n, B, ci, co, g, tuple(S), tuple(k), tuple(stride or (1,) * n), tuple(pad or (0,) * n),
            tuple(dil or (1,) * n), mode, True, 0, transposed, tuple(out_pad or (0,) * n), F64)


def _axis(Sp, Lf, kd):
    """The planner's rule: nextpow2(Sp) <= 2048 as one transform, or overlap-save tiles of T >= 2 kd or 2048 points;
    fewest n*T points, the shorter tile on a tie."""
    cands = []
    t = 8
    while t < Sp:
        t *= 2
    if t <= 2048:
        cands.append(t)
    cands += [T for T in (8, 16, 32, 64, 128, 256, 512, 1024, 2048) if T >= 2 * kd or T == 2048]
    best = min(((-(-Lf // (T - kd + 1))) * T, T) for T in set(cands) if T - kd + 1 >= 1)
    T = best[1]
    V = T - kd + 1
    return T, V, -(-Lf // V)


def _expect(B, ci, co, g, S, k, stride, pad, dil, transposed=False, out_pad=None):
    n = len(S)
    geo = []
    for i in range(n):
        kd = (k[i] - 1) * dil[i] + 1
        if transposed:
            out = (S[i] - 1) * stride[i] - 2 * pad[i] + kd - 1 + out_pad[i] + 1
            Lf, Sp, O = out, out + kd - 1, out
        else:
            Sp = S[i] + 2 * pad[i]
            Lf = Sp - kd + 1
            O = (Lf - 1) // stride[i] + 1
        geo.append(_axis(Sp, Lf, kd) + (O,))
    cig, cog = ci // g, co // g
    Tx = geo[-1][0]
    Fx = Tx // 2 + 1
    ncol = geo[-1][2] * Fx
    t_outer = geo[0][0] * (geo[1][0] if n == 3 else 1)
    spectrum = g * cog * cig * t_outer * Fx * C2
    na = co * cig
    if n == 2:
        a = max(B * ci * S[0] * ncol, na * k[0] * Fx)
        b = B * co * geo[0][3] * ncol
    else:
        mcol = geo[1][2] * geo[1][0] * ncol
        a = max(B * ci * S[0] * S[1] * ncol, na * k[0] * k[1] * Fx, B * co * geo[0][3] * mcol)
        b = max(B * ci * S[0] * mcol, na * k[0] * geo[1][0] * Fx, B * co * geo[0][3] * geo[1][3] * ncol)
    layout = (geo[0][0], Tx, geo[1][0] if n == 3 else 0, 0, 0, 0, 0, 0)
    return Tx, layout, spectrum, (a + b) * C2, geo


ND_CASES = [
    # B, Cin, Cout, groups, size, k, stride, padding, dilation
    (4, 8, 8, 1, (256, 256), (15, 15), (1, 1), (7, 7), (1, 1)),            # B4 8->8 256^2 k15^2
    (8, 8, 8, 1, (64, 64, 64), (9, 9, 9), (1, 1, 1), (0, 0, 0), (1, 1, 1)),  # cfgC in float64
    (8, 8, 8, 1, (64, 64, 64), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1)),  # 'same' k3^3
    (3, 36, 9, 3, (29, 31), (7, 9), (2, 3), (3, 1), (1, 1)),               # groups, ragged channels, stride
    (1, 2, 2, 1, (8, 5000), (3, 65), (1, 1), (1, 32), (1, 1)),             # Lf > 2048 along x: tiles
    (1, 1, 2, 1, (40, 1500), (3, 513), (1, 1), (0, 0), (1, 2)),            # dilated extent 1025
    (2, 4, 3, 1, (300, 5, 4), (17, 2, 2), (2, 1, 1), (8, 0, 1), (1, 1, 1)),
    (1, 1, 1, 1, (2500, 10), (513, 3), (1, 1), (0, 0), (2, 1)),            # dilated extent 1025, Sp > 2048: outer axis
    (1, 1, 1, 1, (10, 2500), (3, 513), (1, 1), (0, 0), (1, 2)),            # ... last axis
    (1, 1, 1, 1, (10, 2500), (3, 1025), (1, 1), (0, 0), (1, 1)),
]


@pytest.mark.parametrize("case", ND_CASES, ids=[f"{'x'.join(map(str, c[4]))}-k{'x'.join(map(str, c[5]))}" for c in ND_CASES])
def test_float64_nd_plan_takes_the_fft_path(case, monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    B, ci, co, g, S, k, s, p, d = case
    plan = _native.Plan(_key(B, ci, co, g, S, k, s, p, d))
    Tx, layout, spectrum, workspace, _ = _expect(B, ci, co, g, S, k, s, p, d)
    assert plan.tile == Tx > 0
    assert plan.layout == layout
    assert plan.spectrum_bytes == spectrum
    assert plan.workspace_bytes == workspace


TR_CASES = [
    # B, Cin, Cout, groups, size, k, stride, padding, dilation, output_padding
    (2, 120, 6, 2, (9, 11), (3, 4), (2, 3), (1, 2), (3, 1), (2, 1)),
    (1, 32, 16, 1, (64, 64), (4, 4), (2, 2), (1, 1), (1, 1), (0, 0)),     # stride-2 decoder layer
    (2, 24, 4, 1, (5, 6, 7), (3, 2, 3), (2, 1, 2), (1, 0, 2), (1, 2, 4), (1, 0, 3)),
]


@pytest.mark.parametrize("case", TR_CASES, ids=[f"{len(c[4])}d-{'x'.join(map(str, c[4]))}" for c in TR_CASES])
def test_float64_transposed_plan_takes_the_fft_path(case, monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    B, ci, co, g, S, k, s, p, d, op = case
    plan = _native.Plan(_key(B, ci, co, g, S, k, s, p, d, transposed=True, out_pad=op))
    Tx, layout, spectrum, workspace, _ = _expect(B, ci, co, g, S, k, s, p, d, transposed=True, out_pad=op)
    assert plan.tile == Tx > 0
    assert plan.layout == layout
    assert plan.spectrum_bytes == spectrum
    assert plan.workspace_bytes == workspace


def test_float64_1d_transposed_plan_takes_the_fft_path(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    plan = _native.Plan(_key(2, 8, 8, 1, (700,), (33,), (2,), (5,), transposed=True, out_pad=(1,)))
    assert plan.tile >= 256 and plan.workspace_bytes == 0
    assert plan.spectrum_bytes == 8 * 8 * plan.tile * C2


def test_float64_long_axis_is_tiled_within_2048_points(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    plan = _native.Plan(_key(1, 2, 2, 1, (8, 5000), (3, 65), pad=(1, 32)))
    assert 0 < plan.tile <= 2048 and plan.layout[1] == plan.tile
    _, _, _, _, geo = _expect(1, 2, 2, 1, (8, 5000), (3, 65), (1, 1), (1, 32), (1, 1))
    assert geo[1][2] > 1                                   # several overlap-save tiles along x
    plan = _native.Plan(_key(1, 4, 2, 1, (3000, 9), (40, 3), (3, 1), (5, 1), mode=1))
    assert 0 < plan.layout[0] <= 2048 and plan.tile > 0


@pytest.mark.parametrize("key", [
    _key(1, 2, 2, 1, (6, 1400), (3, 600), dil=(1, 2)),                   # dilated extent 1199 > 1025
    _key(2, 3, 3, 1, (10, 10), (1, 1)),                                   # 1 x 1 kernel: below the crossover
    _key(2, 3, 3, 1, (5, 6, 7), (1, 1, 1)),
    _key(2, 3, 3, 1, (40,), (15,), transposed=True),                      # 1-D transposed: fewer than 16 taps
    _key(2, 11, 4, 1, (30, 30), (3, 3)),                                  # 99 multiply-adds per output
    _key(2, 3, 4, 1, (10, 10, 10), (2, 3, 5)),                            # 90
], ids=["kd1199", "1x1", "1x1x1", "1d-transposed-k15", "2d-macs99", "3d-macs90"])
def test_float64_direct_kernel_shapes(key, monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    plan = _native.Plan(key)
    _assert_direct(plan, key)


def _assert_direct(plan, key):
    """Direct kernel: no transform anywhere, no workspace, and the "kernel spectrum" is the weight tensor itself."""
    n, _, ci, co, g, _, k = key[:7]
    weight = co * (ci // g) * 8
    for kk in k:
        weight *= kk
    assert plan.tile == 0 and plan.layout[:3] == (0, 0, 0)
    assert plan.workspace_bytes == 0 and plan.spectrum_bytes == weight


def test_float64_launch_past_one_dispatch_keeps_the_direct_kernel(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    key = _key(4096, 64, 64, 1, (4096, 64), (5, 5))          # the row pass alone would need > 2^32 work-items
    _assert_direct(_native.Plan(key), key)


def test_float64_crossover_is_100_multiply_adds_per_output(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    assert _native.Plan(_key(2, 4, 4, 1, (30, 30), (5, 5))).tile > 0                 # 4 x 25 = 100
    assert _native.Plan(_key(2, 12, 4, 4, (30, 30), (5, 5))).tile == 0               # groups: 3 x 25 = 75
    assert _native.Plan(_key(2, 4, 4, 1, (30, 30), (5, 5), transposed=True)).tile > 0
    assert _native.Plan(_key(2, 2, 4, 1, (30,), (16,), transposed=True)).tile > 0   # 1-D: 16 taps
    # a strided forward plan counts per stride-1 output (its FFT computes all of them); a transposed one does not divide
    assert _native.Plan(_key(2, 8, 4, 1, (30, 30), (5, 5), stride=(2, 1))).tile > 0    # 200 / 2 = 100
    assert _native.Plan(_key(2, 4, 4, 1, (30, 30), (5, 5), stride=(2, 1))).tile == 0   # 100 / 2
    assert _native.Plan(_key(2, 4, 4, 1, (30, 30), (5, 5), stride=(2, 2), transposed=True)).tile > 0    # 100
    assert _native.Plan(_key(2, 3, 4, 1, (30, 30), (5, 5), stride=(2, 2), transposed=True)).tile == 0   # 75


def test_float64_knob_keeps_the_direct_kernel(monkeypatch):
    monkeypatch.setenv("FFTCONV_F64_FFT", "0")
    for key in (_key(4, 8, 8, 1, (256, 256), (15, 15), pad=(7, 7)), _key(8, 8, 8, 1, (64, 64, 64), (9, 9, 9)),
                _key(2, 8, 8, 1, (700,), (33,), (2,), (5,), transposed=True, out_pad=(1,))):
        plan = _native.Plan(key)
        assert plan.tile == 0 and plan.workspace_bytes == 0


# ----------------------------------------------------------------------------- Plan.route (fc_debug_route)
def _nb_cob(B, cog, spectrum):
    """plan_nd_f64's channel blocking of the fused pass: 8 output channels a workgroup, spare slots (few output
    channels) or a kernel spectrum of 32 MiB or more make batch items share each read of it."""
    cob, nb = min(8, cog), 1
    if cob <= 2 and B >= 3:
        nb = 4
    elif cob <= 4 and B >= 2:
        nb = 2
    elif spectrum >= 32 << 20 and B >= 2:
        nb, cob = 2, 4
    return nb, cob


ROUTE_CASES = ND_CASES + [
    # B, Cin, Cout, groups, size, k, stride, padding, dilation
    (3, 4, 2, 1, (30, 40), (7, 7), (1, 1), (3, 3), (1, 1)),                 # cob 2, B 3: nb 4
    (7, 6, 2, 1, (8, 10, 12), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1)),  # nb 4, a remainder of 3
    (2, 4, 2, 1, (30, 40), (7, 7), (1, 1), (3, 3), (1, 1)),                 # cob 2, B 2: nb 2
    (2, 9, 4, 1, (21, 33), (7, 7), (2, 2), (3, 3), (1, 1)),                 # cob 4: nb 2
    (1, 4, 3, 1, (30, 40), (7, 7), (1, 1), (3, 3), (1, 1)),                 # B 1: nb 1
    (2, 4, 9, 1, (30, 40), (7, 7), (1, 1), (3, 3), (1, 1)),                 # cob 8, a partial chunk
    # 256 x 256 transforms (248^2 'same', k 9): 528,384 spectrum bytes per channel pair, 63.5 pairs make 32 MiB
    (2, 9, 7, 1, (248, 248), (9, 9), (1, 1), (4, 4), (1, 1)),               # 63 pairs: just below, nb 1
    (2, 8, 8, 1, (248, 248), (9, 9), (1, 1), (4, 4), (1, 1)),               # 64 pairs: just above, nb 2 cob 4
    (1, 8, 8, 1, (248, 248), (9, 9), (1, 1), (4, 4), (1, 1)),               # above, but one batch item: nb 1
    (3, 12, 6, 1, (248, 248), (9, 9), (1, 1), (4, 4), (1, 1)),              # Cout 6 in chunks of 4: the last one partial
    (2, 13, 5, 1, (248, 248), (9, 9), (1, 1), (4, 4), (1, 1)),
]


@pytest.mark.parametrize("case", ROUTE_CASES, ids=[f"B{c[0]}c{c[1]}-{c[2]}-{'x'.join(map(str, c[4]))}-k{'x'.join(map(str, c[5]))}"
                                                   for c in ROUTE_CASES])
def test_float64_nd_route_words(case, monkeypatch):
    """Plan.route of a float64 N-d plan: per-axis transform lengths and tile counts as the axis rule gives them, and the
    fused pass's batch sharing and channel block as plan_nd_f64's rule gives them."""
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    B, ci, co, g, S, k, s, p, d = case
    plan = _native.Plan(_key(B, ci, co, g, S, k, s, p, d))
    _, _, spectrum, _, geo = _expect(B, ci, co, g, S, k, s, p, d)
    r = plan.route
    assert r["kind"] == "f64_fft_nd", r
    n = len(S)
    assert [r[f"t{i}"] for i in range(3)] == [geo[i][0] for i in range(n)] + [0] * (3 - n), r
    assert [r[f"nt{i}"] for i in range(3)] == [geo[i][2] for i in range(n)] + [0] * (3 - n), r
    assert plan.spectrum_bytes == spectrum
    assert (r["nb"], r["cob"]) == _nb_cob(B, co // g, spectrum), (r, spectrum)


def test_float64_32_mib_boundary_both_sides(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    geo = (1, 1), (4, 4), (1, 1)
    below = _native.Plan(_key(2, 9, 7, 1, (248, 248), (9, 9), *geo))
    above = _native.Plan(_key(2, 8, 8, 1, (248, 248), (9, 9), *geo))
    assert below.spectrum_bytes < 32 << 20 <= above.spectrum_bytes
    assert (below.route["nb"], below.route["cob"]) == (1, 7)
    assert (above.route["nb"], above.route["cob"]) == (2, 4)


def test_float64_other_kinds_route_words(monkeypatch):
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    assert _native.Plan(_key(2, 3, 3, 1, (10, 10), (1, 1))).route == {"kind": "f64_direct"}
    plan = _native.Plan(_key(2, 2, 3, 1, (5000,), (600,), pad=(10,)))
    T, V = 2048, 2048 - 600 + 1
    assert plan.route == {"kind": "f64_fft_1d", "T": T, "ntiles": -(-(5000 + 20 - 599) // V), "cob": 2}
    assert plan.tile == T


def test_debug_route_rejects_null_arguments(monkeypatch):
    import ctypes
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    lib = _native.load_library()
    words = (ctypes.c_int32 * 16)()
    assert lib.fc_debug_route(None, ctypes.byref(words)) == _native.FC_ERR_INVALID
    plan = _native.Plan(_key(2, 3, 3, 1, (10, 10), (1, 1)))
    assert lib.fc_debug_route(plan._h, None) == _native.FC_ERR_INVALID
