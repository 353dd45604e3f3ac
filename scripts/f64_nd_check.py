"""float64 2-D / 3-D and transposed convolutions: the FFT path (csrc/nd_f64.hip) against the direct kernel
(FFTCONV_F64_FFT=0) and the reference's torch.fft formulation (rfftn / einsum / irfftn) on the same GPU, plus the
crossover sweep that sets the planner's threshold (kF64MinMacs in csrc/host_f64.cpp).
Usage: python scripts/f64_nd_check.py [--sweep-only | --no-sweep | --cfgc-only]
(the sweep times the FFT path below the crossover too: FFTCONV_F64_FFT=2 plans every shape the path can run)"""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fft_conv_pytorch_amd import _native  # noqa: E402
from fft_conv_pytorch_amd.functional import _plan_for, fft_conv, fft_conv_transpose  # noqa: E402

dev = "cuda:0"


def timed(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def replayed(fn, iters=10, per=2):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    return timed(g.replay, iters) / per


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def torch_fft_conv(x, w, b, padding):
    """The reference's algorithm (functional.py:60-87) in torch.fft: pad, rfftn of signal and zero-padded kernel
    over every spatial axis, per-bin channel contraction, irfftn, crop."""
    n = x.ndim - 2
    flat = [q for p in reversed(padding) for q in (p, p)]
    xp = F.pad(x, flat)
    sp = xp.shape[2:]
    dims = tuple(range(2, 2 + n))
    X = torch.fft.rfftn(xp, dim=dims)
    kp = F.pad(w, [q for i in reversed(range(n)) for q in (0, sp[i] - w.shape[2 + i])])
    H = torch.fft.rfftn(kp, dim=dims).conj()
    Y = torch.einsum("bi...,oi...->bo...", X, H)
    y = torch.fft.irfftn(Y, s=sp, dim=dims)
    crop = (slice(None), slice(None)) + tuple(slice(0, sp[i] - w.shape[2 + i] + 1) for i in range(n))
    return y[crop] + b.view(1, -1, *([1] * n))


def set_knob(v):
    os.environ["FFTCONV_F64_FFT"] = v
    _native.clear_plan_cache()


def forward_row(name, B, ci, co, S, k, padding, direct_iters=1, ref=True):
    n = len(S)
    x = torch.randn(B, ci, *S, device=dev, dtype=torch.float64)
    w = torch.randn(co, ci, *k, device=dev, dtype=torch.float64)
    b = torch.randn(co, device=dev, dtype=torch.float64)
    conv = (F.conv1d, F.conv2d, F.conv3d)[n - 1]
    want = conv(x, w, b, padding=padding)
    set_knob("1")
    plan = _plan_for(x, w, b, 1, padding, 1, 1, "constant")
    y = fft_conv(x, w, b, padding=padding)
    err = rel(y, want)
    t_eager = timed(lambda: fft_conv(x, w, b, padding=padding), 5)
    t_graph = replayed(lambda: fft_conv(x, w, b, padding=padding), 5)
    set_knob("0")
    yd = fft_conv(x, w, b, padding=padding)
    t_direct = timed(lambda: fft_conv(x, w, b, padding=padding), direct_iters, warm=0)
    err_d = rel(yd, want)
    set_knob("1")
    t_ref, err_ref = float("nan"), float("nan")
    if ref:
        yr = torch_fft_conv(x, w, b, padding)
        err_ref = rel(yr, want)
        t_ref = timed(lambda: torch_fft_conv(x, w, b, padding), 5)
    macs = B * co * want[0, 0].numel() * ci * torch.tensor(k).prod().item()
    hbytes = plan.spectrum_bytes
    print(f"{name}: FFT path {t_eager:10.1f} us eager / {t_graph:10.1f} us replayed (T {plan.layout[:3]}, |H| "
          f"{hbytes / 1e6:.1f} MB) | direct {t_direct:12.1f} us ({macs / 1e9:.1f} GMAC, {t_direct / t_graph:.1f}x) | "
          f"torch.fft rfftn {t_ref:10.1f} us ({t_ref / t_graph:.2f}x) | rel err FFT {err:.1e}, direct {err_d:.1e}, "
          f"torch.fft {err_ref:.1e}", flush=True)


def main():
    torch.manual_seed(0)
    if "--cfgc-only" in sys.argv:      # (for a rocprofv3 --kernel-trace --stats run)
        forward_row("cfgC-f64 B8 8->8 64^3 k9^3", 8, 8, 8, (64, 64, 64), (9, 9, 9), (0, 0, 0), direct_iters=1, ref=False)
        return
    sweep_only = "--sweep-only" in sys.argv
    if not sweep_only:
        forward_row("B4 8->8 256^2 k15^2", 4, 8, 8, (256, 256), (15, 15), (0, 0), direct_iters=2)
        forward_row("cfgB-f64 B16 8->8 512^2 k31^2", 16, 8, 8, (512, 512), (31, 31), (0, 0), direct_iters=1)
        forward_row("cfgC-f64 B8 8->8 64^3 k9^3", 8, 8, 8, (64, 64, 64), (9, 9, 9), (0, 0, 0), direct_iters=1)
        forward_row("B8 8->8 64^3 k3^3 same", 8, 8, 8, (64, 64, 64), (3, 3, 3), (1, 1, 1), direct_iters=2)
        # 2-D stride-2 transposed decoder layer
        x = torch.randn(8, 32, 64, 64, device=dev, dtype=torch.float64)
        w = torch.randn(32, 16, 4, 4, device=dev, dtype=torch.float64)
        b = torch.randn(16, device=dev, dtype=torch.float64)
        want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
        call = lambda: fft_conv_transpose(x, w, b, stride=2, padding=1)  # noqa: E731
        set_knob("1")
        plan = _plan_for(x, w, b, 2, 1, 1, 1, "constant", transposed=True)
        err = rel(call(), want)
        te, tg = timed(call, 5), replayed(call, 5)
        set_knob("0")
        td = timed(call, 3, warm=1)
        set_knob("1")
        tt = timed(lambda: F.conv_transpose2d(x, w, b, stride=2, padding=1), 5)
        print(f"decoder B8 32->16 64^2 k4 s2 transposed: FFT path {te:.1f} us eager / {tg:.1f} us replayed "
              f"(T {plan.layout[:3]}) | direct {td:.1f} us ({td / tg:.1f}x) | torch conv_transpose2d {tt:.1f} us | "
              f"rel err {err:.1e}", flush=True)
        # one float64 FFTConv2d training step (forward + backward)
        from fft_conv_pytorch_amd import FFTConv2d
        for knob in ("1", "0"):
            set_knob(knob)
            layer = FFTConv2d(8, 8, 15, padding=7, bias=True).to(dev).double()
            xs = torch.randn(4, 8, 128, 128, device=dev, dtype=torch.float64, requires_grad=True)

            def step():
                layer.zero_grad(set_to_none=True)
                xs.grad = None
                layer(xs).square().sum().backward()
            t = timed(step, 5 if knob == "1" else 2, warm=1)
            print(f"train step FFTConv2d 8->8 k15 'same' B4 128^2 ({'FFT path' if knob == '1' else 'direct kernel'}): "
                  f"{t:.1f} us", flush=True)
        set_knob("1")
    if "--no-sweep" in sys.argv:
        return
    # crossover: 2-D B4 Cig->8 128^2 and 3-D B2 Cig->8 32^3, 'same'-style padding, k in {2, 3, 5, 7}
    print("crossover sweep (replayed us; macs = Cig * prod(k) per output)", flush=True)
    for nd, B, S in ((2, 4, (128, 128)), (3, 2, (32, 32, 32))):
        for cig in (1, 8):
            for k in (2, 3, 5, 7):
                x = torch.randn(B, cig, *S, device=dev, dtype=torch.float64)
                w = torch.randn(8, cig, *([k] * nd), device=dev, dtype=torch.float64)
                b = torch.randn(8, device=dev, dtype=torch.float64)
                pad = (k // 2,) * nd
                call = lambda: fft_conv(x, w, b, padding=pad)  # noqa: E731
                set_knob("2")
                plan = _native.Plan((nd, B, cig, 8, 1, S, (k,) * nd, (1,) * nd, pad, (1,) * nd, 0, True, 0, False,
                                     (0,) * nd, 1))
                t_fft = float("nan")
                if plan.tile:
                    t_fft = replayed(call, 5)
                set_knob("0")
                t_dir = replayed(call, 5)
                set_knob("1")
                print(f"  {nd}-D B{B} {cig}->8 {S[0]}^{nd} k{k}: macs {cig * k ** nd:5d}  FFT {t_fft:10.1f}  "
                      f"direct {t_dir:10.1f}  ratio {t_dir / t_fft:.2f}", flush=True)
    # strided 2-D rows, forward (the FFT path computes every stride-1 output) and transposed: macs / prod(stride)
    print("strided crossover rows (2-D B4, stride 2 x 2; macs = Cig * prod(k) / 4)", flush=True)
    for transposed, cig, k in ((False, 8, 3), (False, 8, 5), (False, 8, 7), (False, 8, 9), (False, 16, 7),
                               (True, 8, 4), (True, 8, 6), (True, 8, 8), (True, 16, 8)):
        S = (64, 64) if transposed else (128, 128)
        x = torch.randn(4, cig, *S, device=dev, dtype=torch.float64)
        if transposed:
            w = torch.randn(cig, 8, k, k, device=dev, dtype=torch.float64)
            call = lambda: fft_conv_transpose(x, w, None, stride=2, padding=k // 2 - 1)  # noqa: E731
        else:
            w = torch.randn(8, cig, k, k, device=dev, dtype=torch.float64)
            call = lambda: fft_conv(x, w, None, stride=2, padding=k // 2)  # noqa: E731
        set_knob("2")
        t_fft = replayed(call, 5)
        set_knob("0")
        t_dir = replayed(call, 5)
        set_knob("1")
        print(f"  {'transposed' if transposed else 'forward   '} {cig}->8 {S[0]}^2 k{k} s2: macs/stride "
              f"{cig * k * k // 4:5d}  FFT {t_fft:10.1f}  direct {t_dir:10.1f}  ratio {t_dir / t_fft:.2f}", flush=True)
    os.environ.pop("FFTCONV_F64_FFT", None)


if __name__ == "__main__":
    main()
