"""``fft_long_conv`` / ``FFTLongConv1d`` on the GPU: one transform over the whole padded row in three launches
(csrc/long1d.hpp).  Every factorisation N1 x N2 is checked against the float64 oracle on CPU copies, error
max|got - want| / max|want| within route_util.TOL32; seams, large rows (sampled float64 dot products), agreement with the
segment route of ``fft_conv``, the three gradients, the module and graph capture follow."""
import copy
import pickle

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, fft_conv, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from oracle.fft_conv_oracle import fft_conv_oracle_torch
from tests.route_util import TOL32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fresh_plans(monkeypatch):
    """FFTCONV_LONG_N is read at plan creation and is not part of the cache key."""
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    monkeypatch.delenv("FFTCONV_LONG_WS_MB", raising=False)
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


def _err(got, want):
    return (got.double().cpu() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)


def _want(x, w, b, padding, groups, causal):
    """The oracle on float64 CPU copies; causal: on the left-padded row and the flipped kernel."""
    x, w = x.double().cpu(), w.double().cpu()
    b = None if b is None else b.double().cpu()
    if causal:
        return fft_conv_oracle_torch(F.pad(x, (w.shape[2] - 1, 0)), w.flip(-1), b, groups=groups)
    if isinstance(padding, str):
        return F.conv1d(x, w, b, padding=padding, groups=groups)      # (the oracle takes numbers; torch's float64 conv1d)
    return fft_conv_oracle_torch(x, w, b, padding=padding, groups=groups)


def _tensors(B, cin, cout, g, L, K, bias, seed=0):
    gen = torch.Generator().manual_seed(seed + L + 3 * K)
    x = torch.randn(B, cin, L, generator=gen).to(DEV)
    w = torch.randn(cout, cin // g, K, generator=gen).to(DEV)
    b = torch.randn(cout, generator=gen).to(DEV) if bias else None
    return x, w, b


def _factors(L, K, padding, causal):
    pl, pr, _ = F_._long_geometry(torch.empty(1, 1, L), torch.empty(1, 1, K), None, padding, 1, causal)
    info = _native.long_geometry((1, 1, 1, 1, L, K, pl, pr, L if causal else 0, int(causal), 0))
    return info["N1"], info["N2"]


def _check(B, cin, cout, g, L, K, padding, causal, bias, expect=None):
    x, w, b = _tensors(B, cin, cout, g, L, K, bias)
    if expect is not None:
        assert _factors(L, K, padding, causal) == expect
    got = fft_long_conv(x, w, b, padding=padding, groups=g, causal=causal)
    want = _want(x, w, b, padding, g, causal)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = _err(got, want)
    print(f"long B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} bias={bias} N={expect}: err {err:.2e}")
    assert err <= TOL32
    return x, w, b, want


# what the planner picks up to N = 2^16: exactly filled, and one sample past the factorisation before
PLANNER_CASES = [
    # B, cin, cout, g, L, K, padding, causal, bias, (N1, N2)
    (1, 4, 4, 4, 4097, 1, 0, True, True, (64, 128)),             # one past 64 x 64, K = 1
    (2, 3, 5, 1, 4100, 2, 0, True, False, (64, 128)),            # K = 2, g = 1 with Cin != Cout
    (3, 4, 4, 4, 4096, 4096, 0, True, True, (64, 128)),          # K = L: 8191 points
    (5, 6, 4, 2, 4097, 4096, 0, True, False, (64, 128)),         # K = L - 1: 8192, exactly filled; 1 < g < C
    (2, 2, 2, 2, 4097, 4097, 0, True, True, (128, 128)),         # one past: 8193
    (3, 2, 2, 1, 5000, 5007, 0, True, True, (128, 128)),         # K = L + 7
    (2, 2, 2, 2, 3000, 6000, 0, True, False, (64, 128)),         # K = 2L
    (1, 4, 6, 2, 16384, 33, 0, False, True, (128, 128)),         # padding 0: exactly 2^14
    (2, 4, 4, 4, 16385, 33, 0, False, False, (128, 256)),        # one past
    (3, 2, 2, 1, 20000, 4001, 2000, False, True, (128, 256)),    # padding K // 2
    (2, 3, 3, 3, 32768, 2000, "valid", False, False, (128, 256)),
    (5, 2, 4, 2, 30000, 3000, "same", False, True, (256, 256)),  # 'same' with an even kernel
    (2, 2, 2, 2, 32769, 32768, 0, True, True, (256, 256)),       # 2^16 exactly filled
    (1, 1, 1, 1, 65536, 1, 0, False, False, (256, 256)),
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,bias,expect", PLANNER_CASES)
def test_parity_for_every_factorisation_the_planner_picks(B, cin, cout, g, L, K, padding, causal, bias, expect):
    _check(B, cin, cout, g, L, K, padding, causal, bias, expect)


# every tile length on each side at least once
FORCED = [(64, 64), (128, 64), (256, 64), (512, 64), (1024, 64), (2048, 64), (4096, 64),
          (64, 256), (64, 512), (64, 1024), (64, 2048), (64, 4096), (512, 512), (1024, 128)]


@pytest.mark.parametrize("N1,N2", FORCED)
def test_parity_and_full_coverage_for_forced_factorisations(N1, N2, monkeypatch):
    """Small shapes through FFTCONV_LONG_N; the C-level forward into a NaN-filled output writes every sample."""
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _native.clear_plan_cache()
    B, cin, cout, g, L, K = 3, 4, 6, 2, (2500 if N1 * N2 == 4096 else 3000), 1500      # (4096 points: C level only)
    causal = (N1 + N2) % 3 != 0
    padding = 0 if causal else 700
    x, w, b, want = _check(B, cin, cout, g, L, K, padding, causal, True, (N1, N2))
    pl, pr = (K - 1, 0) if causal else (padding, padding)
    plan = F_._long_plan(x, cout, g, K, pl, pr, causal, L if causal else 0, True)
    assert (plan.info["N1"], plan.info["N2"]) == (N1, N2)
    spectrum = F_.transform_kernel(plan, w)
    out = torch.full((B, cout, plan.out_len), float("nan"), device=DEV)
    ws = F_.new_workspace(plan, x.device)
    plan.forward(x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    assert _err(out, want) <= TOL32


def test_slabs_of_batch_pairs_match_one_slab(monkeypatch):
    x, w, b = _tensors(7, 4, 4, 4, 16000, 9000, True)
    one = fft_long_conv(x, w, b, groups=4, causal=True)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "3")        # 32768 points x 8 channels x 8 bytes = 2 MiB per pair
    _native.clear_plan_cache()
    plan = F_._long_plan(x, 4, 4, 9000, 8999, 0, True, 16000, True)
    assert plan.info["slabs"] == 4 and plan.info["slab_pairs"] == 1
    assert torch.equal(fft_long_conv(x, w, b, groups=4, causal=True), one)
    assert _err(one, _want(x, w, b, 0, 4, True)) <= TOL32


@pytest.mark.parametrize("L,K", [(20000, 20000), (5000, 3000)])
def test_seams(L, K):
    """Unit impulses at the row ends and on both sides of the first row boundaries of the N1 x N2 layout against a ramp
    kernel: output t of the causal form is ramp[t - position], compared in position."""
    N1, N2 = _factors(L, K, 0, True)
    spots = [0, L - 1, N2 - 1, N2, 2 * N2 - 1, 2 * N2]
    x = torch.zeros(len(spots), 1, L, device=DEV)
    for i, s in enumerate(spots):
        x[i, 0, s] = 1.0
    ramp = (torch.arange(K, dtype=torch.float32, device=DEV) + 1.0) / K
    got = fft_long_conv(x, ramp.view(1, 1, K), causal=True)
    t = torch.arange(L, device=DEV)
    for i, s in enumerate(spots):
        lag = t - s
        want = torch.where((lag >= 0) & (lag < K), ramp[lag.clamp(0, K - 1)], torch.zeros((), device=DEV))
        err = (got[i, 0] - want).abs().max().item()
        # (relative to max|want| over the batch, which is 1: two batch items share one complex transform, so the rounding
        # of a row scales with its partner's magnitude too)
        assert err <= TOL32, (s, err)


@pytest.mark.parametrize("L,K,expect", [(1 << 19, 1 << 19, (1024, 1024)), ((1 << 20) - 5, (1 << 19) + 6, (1024, 2048))])
def test_large_rows_on_sampled_float64_dot_products(L, K, expect):
    B, C = 3, 4
    assert _factors(L, K, 0, True) == expect
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(B, C, L, generator=gen).to(DEV)
    w = (torch.randn(C, 1, K, generator=gen) / 64).to(DEV)
    b = torch.randn(C, generator=gen).to(DEV)
    got = fft_long_conv(x, w, b, groups=C, causal=True)
    assert got.shape == (B, C, L)
    spots = list(range(8)) + list(range(L - 8, L)) + torch.randint(8, L - 8, (4096 - 16,), generator=gen).tolist()
    x64, wf = x.double(), w.double().flip(-1)[:, 0]           # wf[c, K - 1 - s] = w[c, s]
    want = torch.empty(B, C, len(spots), dtype=torch.float64, device=DEV)
    for j, t in enumerate(spots):
        lo = max(0, t - K + 1)
        want[:, :, j] = (x64[:, :, lo:t + 1] * wf[None, :, K - 1 - t + lo:K]).sum(-1) + b.double()
    sel = got[:, :, torch.tensor(spots, device=DEV)].double()
    err = (sel - want).abs().max().item() / want.abs().max().item()
    print(f"long causal depthwise B{B} C{C} L{L} K{K}: sampled err {err:.2e}")
    assert err <= TOL32


def test_agrees_with_the_segment_route_of_fft_conv():
    x, w, b = _tensors(4, 8, 8, 1, 8192, 8192, True)
    new = fft_long_conv(x, w, b, padding=4096)
    old = fft_conv(x, w, b, padding=4096)
    assert new.shape == old.shape
    assert (new - old).abs().max().item() <= 2 * TOL32 * old.abs().max().item()


def test_short_rows_run_the_fft_conv_kernels():
    _check(2, 4, 4, 2, 3000, 500, 200, False, True)
    _check(3, 2, 2, 2, 1500, 2000, 0, True, True)


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal", [
    (3, 4, 4, 4, 5000, 5000, 0, True),
    (2, 6, 4, 2, 7000, 3000, 100, False),
    (2, 2, 2, 1, 3000, 6000, 0, True),
])
def test_gradients_match_float64_autograd_through_the_oracle(B, cin, cout, g, L, K, padding, causal):
    x, w, b = _tensors(B, cin, cout, g, L, K, True)
    x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    y = fft_long_conv(x, w, b, padding=padding, groups=g, causal=causal)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    y.backward(gy)
    xc, wc, bc = (t.detach().double().cpu().requires_grad_() for t in (x, w, b))
    if causal:
        ref = fft_conv_oracle_torch(F.pad(xc, (K - 1, 0)), wc.flip(-1), bc, groups=g)
    else:
        ref = fft_conv_oracle_torch(xc, wc, bc, padding=padding, groups=g)
    ref.backward(gy.double().cpu())
    errs = {"y": _err(y.detach(), ref.detach()), "dX": _err(x.grad, xc.grad), "dW": _err(w.grad, wc.grad),
            "db": _err(b.grad, bc.grad)}
    print(f"long grads L{L} K{K} causal={causal}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert x.grad.shape == x.shape and w.grad.shape == w.shape
    for name, err in errs.items():
        assert err <= TOL32, (name, err)


def test_module_state_dict_cache_and_copies(monkeypatch):
    torch.manual_seed(0)
    conv = torch.nn.Conv1d(4, 4, 3001, padding=1500, groups=2).to(DEV)
    layer = FFTLongConv1d(4, 4, 3001, padding=1500, groups=2).to(DEV)
    layer.load_state_dict(conv.state_dict())
    conv.load_state_dict(layer.state_dict())
    x = torch.randn(3, 4, 6000, device=DEV)
    want = _want(x, layer.weight.detach(), layer.bias.detach(), 1500, 2, False)

    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(1) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert len(calls) == 1 and torch.equal(y1, y2) and _err(y1, want) <= TOL32
    with torch.no_grad():
        layer.weight.mul_(0.5)              # bumps the version counter
        y3 = layer(x)
    assert len(calls) == 2
    assert _err(y3, _want(x, layer.weight.detach(), layer.bias.detach(), 1500, 2, False)) <= TOL32
    layer.weight.data.mul_(2.0)             # invisible to the version counter
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y4 = layer(x)
    assert len(calls) == 3 and _err(y4, want) <= TOL32
    layer.train()                           # a training step re-transforms on every call
    layer(x), layer(x)
    assert len(calls) == 5

    layer.eval()
    with torch.no_grad():
        layer(x)
    clone, pickled = copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))
    for other in (clone, pickled):
        assert "_spectrum_cache" not in other.__dict__ and other.causal is False
        with torch.no_grad():
            assert torch.equal(other(x), y4)

    causal = FFTLongConv1d(2, 2, 9000, groups=2, causal=True, bias=False).to(DEV).eval()
    xc = torch.randn(2, 2, 7000, device=DEV)
    with torch.no_grad():
        assert _err(causal(xc), _want(xc, causal.weight.detach(), None, 0, 2, True)) <= TOL32


def test_warm_forward_is_capturable_and_replays_bit_for_bit():
    x, w, b = _tensors(3, 4, 4, 4, 20000, 20000, True)
    plan = F_._long_plan(x, 4, 4, 20000, 19999, 0, True, 20000, True)
    assert plan.info["slabs"] == 1          # one chain of three launches on the capturing stream
    spectrum = F_.transform_kernel(plan, w)
    static_x = x.clone()
    fft_long_conv(static_x, w, b, groups=4, causal=True)       # warm: plan and device tables exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = F_._long_run(static_x, w, b, 19999, 0, True, 20000, 4, spectrum)
    for seed in (1, 2, 3):
        fresh = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = F_._long_run(fresh, w, b, 19999, 0, True, 20000, 4, spectrum)
        assert torch.equal(static_y, eager)
