"""``functional._long_forward_plan`` on the GPU: the module, the functional and the autograd function of ``fft_long_conv``
map a forward route to its plan in that one place, so the spectrum ``FFTLongConv1d`` caches is the spectrum of the plan
the launch runs on -- with and without gradients, on the plain route and by phases -- and the weight is transformed once."""
import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_WGRAD", "FFTCONV_LONG_N",
         "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO", "FFTCONV_TILE")


def _clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@pytest.fixture
def ran(monkeypatch):
    """The long plans whose forward ran, one per launch."""
    seen = []
    real, real_lay = _native.LongPlan.forward, _native.LongPlan.forward_lay

    def forward(plan, *args):
        seen.append(plan)
        return real(plan, *args)

    def forward_lay(plan, *args):
        seen.append(plan)
        return real_lay(plan, *args)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    monkeypatch.setattr(_native.LongPlan, "forward_lay", forward_lay)
    return seen


# B = 2, Cin = Cout = 2, K = 3; a real row of 4100 points is just past the 4096-point handoff, a complex row never hands off
@pytest.mark.parametrize("route,dtype,length", [
    ("plain", torch.float32, 4100),
    ("phases", torch.float32, 4100),
    ("plain", torch.complex64, 64),
])
def test_the_module_caches_the_spectrum_of_the_plan_that_runs(route, dtype, length, ran, monkeypatch):
    stride = 2 if route == "phases" else 1
    if route == "phases":
        monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    assert F_._long_route((2, 2, length), (2, 2, 3), stride=stride, dtype=dtype) == route
    torch.manual_seed(5)
    layer = FFTLongConv1d(2, 2, 3, stride=stride, device=DEV, dtype=dtype).eval()
    x = torch.randn(2, 2, length, device=DEV, dtype=dtype)

    transforms, asked = [], []
    real_transform, real_cached = F_.transform_kernel, FFTLongConv1d._cached_spectrum

    def transform(plan, kernel):
        transforms.append(plan)
        return real_transform(plan, kernel)

    def cached(self, plan, prepare=None):
        asked.append(plan)
        return real_cached(self, plan, prepare)
    monkeypatch.setattr(F_, "transform_kernel", transform)
    monkeypatch.setattr(FFTLongConv1d, "_cached_spectrum", cached)

    with torch.no_grad():
        y0 = layer(x)
    xg = x.clone().requires_grad_(True)
    y1 = layer(xg)
    assert y1.requires_grad
    assert len(transforms) == 1, "the weight was transformed again: the cached spectrum was not the launch's plan's"
    assert len(asked) == 2 and len(ran) == 2
    for want, got in zip(asked, ran):
        assert got is want
        assert type(got) is (_native.LongDecimPlan if route == "phases" else _native.LongPlan)
    assert asked[0] is asked[1] and got.complex == dtype.is_complex
    # the functional on the same tensors: the same plan, the same bits
    with torch.no_grad():
        want0 = fft_long_conv(x, layer.weight, layer.bias, stride=stride)
    want1 = fft_long_conv(xg, layer.weight, layer.bias, stride=stride)
    assert ran[2] is ran[3] is asked[0]
    for y, want in ((y0, want0), (y1, want1)):
        assert y.dtype == dtype and y.shape == want.shape
        assert torch.equal(torch.view_as_real(y) if dtype.is_complex else y,
                           torch.view_as_real(want) if dtype.is_complex else want)
