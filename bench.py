#!/usr/bin/env python3
"""Headline benchmark: forward FFT convolution throughput on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfgA] [--dump-outputs DIR] [--full]

A "step" is one forward pass of the hot path (FFTConv1d.forward, kernel spectrum
cached per weight version as the module does) over one synthetic batch that is
already resident in HBM.  Steps rotate over several distinct input/output
buffer sets whose total size exceeds the 256 MiB Infinity Cache, so every step
streams its input from HBM instead of re-reading a cache-resident copy.  The
steps are captured into a HIP graph (one rotation per graph) to keep the host
out of the timed region; every captured step is a full launch.

N > 1: one process per GPU (torch.distributed, backend nccl = RCCL); each rank
convolves its own batch shard of the same size (weak scaling); the only
collective is the one-off broadcast of the weights from rank 0.  The timed
region is bracketed by barrier + synchronize and the max over ranks is taken.

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0) with the headline
figure (`value`, `ms_per_step`).  `--dump-outputs DIR` writes what the last timed step computed to DIR
(inputs are seeded, so two builds can be compared output for output).  `--full` adds everything else the
benchmark reports: the check of the timed result against an eager forward, the HBM roofline, the eager
end-to-end timings and the CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# name: (ndim, batch, cin, cout, groups, spatial, kernel, dilation)  -- SURVEY.md section 8d
CONFIGS = {
    "cfg0": (1, 1, 8, 8, 1, (32768,), (128,), 1),
    "cfgA": (1, 32, 8, 8, 1, (32768,), (512,), 1),
    "cfgB": (2, 16, 8, 8, 1, (512, 512), (31, 31), 1),
    "cfgC": (3, 8, 8, 8, 1, (64, 64, 64), (9, 9, 9), 1),
    "cfgD": (1, 8, 64, 64, 8, (1 << 20,), (257,), 4),     # per-GPU shard of cfgD (B=64 over 8 GPUs)
    # what ONE GPU of an 8-GPU node runs when the BASELINE.json problems are split over the node (strong scaling):
    "cfgA_shard": (1, 4, 8, 8, 1, (32768,), (512,), 1),           # configs[1]: B=32 over 8 GPUs
    "cfgB_shard": (2, 2, 8, 8, 1, (512, 512), (31, 31), 1),       # configs[2]: B=16 over 8 GPUs
    "cfgC_shard": (3, 1, 8, 8, 1, (64, 64, 64), (9, 9, 9), 1),    # configs[3]: one batch item per GPU
    # the reference's README benchmark shapes (doc/scripts/generate_benchmark_plot.py:128-159: batch 2, 8->8)
    "readme1d": (1, 2, 8, 8, 1, (32768,), (512,), 1),
    "readme2d": (2, 2, 8, 8, 1, (512, 512), (22, 22), 1),
    "readme3d": (3, 2, 8, 8, 1, (64, 64, 64), (8, 8, 8), 1),
}
# whole-node batch of the problems BASELINE.json states for 8 GPUs (--scaling strong splits THIS batch over the ranks)
STRONG_BATCH = {"cfgA": 32, "cfgB": 16, "cfgC": 8, "cfgD": 64}
HBM_PEAK_GBPS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec
DUMP_FULL_BYTES = 48 * 10**6    # --dump-outputs: outputs up to this size are written whole ...
DUMP_SAMPLES = 1 << 21          # ... larger ones as this many elements at fixed, seeded positions


def algorithmic_bytes(batch, cin, cout, groups, spatial, kernel, out_spatial):
    """4*(input + weight + bias + output elements): SURVEY.md section 8d."""
    n_in = batch * cin
    n_out = batch * cout
    for s in spatial:
        n_in *= s
    for s in out_spatial:
        n_out *= s
    n_w = cout * (cin // groups)
    for k in kernel:
        n_w *= k
    return 4 * (n_in + n_w + cout + n_out), n_out


def pmc_traffic(config_name, kernel_name):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (collected
    separately: counters cannot be read from inside the timed run).  Keyed on the workload AND the name of
    the kernel the plan actually launches, so a different tile / kernel variant reads as "not measured"
    (None) instead of inheriting another kernel's counters.  Newest profile round wins."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")), reverse=True):
        try:
            with open(path) as fh:
                prof = json.load(fh)
        except Exception:
            continue
        for entry in prof.get("entries", [prof]):
            if entry.get("workload") == config_name and kernel_name and kernel_name in entry.get("kernel", ""):
                # a forward of several launches (2-D / 3-D): the traffic of all of them, as `achieved` is over all of them
                return entry.get("whole_forward_traffic_bytes", entry.get("traffic_bytes_per_launch"))
    return None


def dominant_kernel_name(plan):
    """Name prefix of the kernel that dominates this plan's forward (as rocprofv3 prints it)."""
    tile, ph, nseg, seg_taps, diag, bd_gs, wide, pers_nb = plan.layout
    if plan.key[0] != 1 and pers_nb:         # (N-d plans report their pipeline in this word: 1 = 3-D plane-major, 2 = 2-D rows as they are)
        return "colz_kernel<"                # the thread-per-sequence column pass + channel mix is the longest launch of both
    if plan.key[0] != 1:
        return "fusedc_kernel"
    geo = {64: (8, 1), 128: (8, 2), 256: (16, 1), 512: (16, 2), 1024: (32, 1), 2048: (32, 2), 4096: (32, 4)}.get(tile)
    if geo is None:
        return None
    if wide == 2:
        return "dense_gemm_kernel<"          # many-channel pipeline: the per-bin GEMM is its longest launch
    if wide:
        return f"conv1d_wide_kernel<{geo[0]}, {geo[1]},"
    if pers_nb:
        return f"conv1d_pers_kernel<{geo[0]}, {geo[1]}, 8, {pers_nb},"
    return f"conv1d_fused_kernel<{geo[0]}, {geo[1]},"


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, budget_s=14.0, budget_1t_s=8.0):
    """The reference's CPU op sequence (oracle/fft_conv_oracle.py, torch CPU backend) timed on this
    host's cores on a bounded sample: whole batches of the same workload until the budget is spent
    (all the cores of this process's CPU share), then a shorter single-thread run."""
    from oracle.fft_conv_oracle import fft_conv_oracle_torch
    ndim, batch, cin, cout, groups, spatial, kernel, dil = cfg
    b = min(batch, 32)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(b, cin, *spatial, generator=g)
    w = torch.randn(cout, cin // groups, *kernel, generator=g)
    bias = torch.randn(cout, generator=g)
    # the GPU box shares its host: use this process's CPU share, not every core of the machine
    cores = max(1, min(len(os.sched_getaffinity(0)), int(os.environ.get("FFTCONV_CPU_THREADS", "16"))))

    def timed(threads, budget, max_passes):
        torch.set_num_threads(threads)
        y = fft_conv_oracle_torch(x, w, bias, dilation=dil, groups=groups)    # warm-up
        times = []
        t_end = time.perf_counter() + budget
        while (time.perf_counter() < t_end and len(times) < max_passes) or not times:
            t0 = time.perf_counter()
            fft_conv_oracle_torch(x, w, bias, dilation=dil, groups=groups)
            times.append(time.perf_counter() - t0)
        return y.numel(), sorted(times)

    # thread sweep (torch's batched complex matmul over 16385 tiny bins does not scale monotonically: on the round-2 host
    # one thread beat sixteen): 1, 8, 16, 32, 64 threads where the host offers them, a bounded budget each; `value` is the
    # best of them with its core count, every point is reported
    visible = len(os.sched_getaffinity(0))
    sweep = sorted({t for t in (1, 8, cores, 32, 64) if t <= max(visible, 1)})
    per_point = max(2.0, (budget_s + budget_1t_s) / len(sweep))
    tried = {}
    n_out = None
    for t in sweep:
        n_out, tt = timed(t, per_point, 40 if t > 1 else 5)
        tried[t] = tt
    threads = min(tried, key=lambda t: tried[t][0])
    pick = tried[threads]
    best, med = pick[0], pick[len(pick) // 2]
    return {"value": n_out / best / 1e9, "unit": "GSamples/s", "cores": threads, "kind": "port",
            "sample": f"{len(pick)} passes of batch {b} of the same workload at {threads} thread(s), best-of; "
                      f"torch {torch.__version__} CPU ops; thread counts tried: {sweep}",
            "ms_per_pass": best * 1e3, "median_value": n_out / med / 1e9, "median_ms_per_pass": med * 1e3,
            "threads_tried": {str(t): {"best_ms": tt[0] * 1e3, "median_ms": tt[len(tt) // 2] * 1e3, "passes": len(tt)}
                              for t, tt in tried.items()},
            "one_thread_value": n_out / tried[1][0] / 1e9,
            "cpu_model": cpu_model(), "host_cores_visible": visible}


def eager_us(fn, iters=60, warm=10):
    """Host-launched (no graph) time per call in microseconds: HIP events around `iters` calls on the current stream."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / iters
    return e0.elapsed_time(e1) * 1e3 / iters, wall


def dump_outputs(out_dir, y):
    """Write the output of the timed path's last step as ``out_dir/y.npy`` (float32, its own shape).  An output
    larger than DUMP_FULL_BYTES is written as DUMP_SAMPLES elements at fixed positions of the flattened tensor
    (seed 0, ascending), ``y.npy``, with those positions as ``y_index.npy`` (float64): about 25 MB in all."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    flat = y.detach().reshape(-1)
    if flat.numel() * flat.element_size() <= DUMP_FULL_BYTES:
        np.save(os.path.join(out_dir, "y.npy"), y.detach().cpu().numpy().astype(np.float32))
        return
    idx = np.sort(np.random.default_rng(0).choice(flat.numel(), size=DUMP_SAMPLES, replace=False))
    sample = flat[torch.from_numpy(idx).to(flat.device)]
    np.save(os.path.join(out_dir, "y.npy"), sample.cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "y_index.npy"), idx.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", default="cfgA", choices=sorted(CONFIGS))
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs the config's batch (per-GPU work fixed); strong: the whole-node batch of the "
                         "BASELINE.json problem (cfgA 32, cfgB 16, cfgC 8, cfgD 64) is split over the ranks with shard_range "
                         "and `value` is the whole problem's outputs per second")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a HIP graph")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: check the timed result against an eager forward, report the HBM "
                         "roofline, the eager end-to-end timings and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the output of the last one to DIR/y.npy (rank 0; a seeded sample "
                         "with DIR/y_index.npy when the output is larger than 48 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-end-to-end", action="store_true",
                    help="with --full: skip the eager module / uncached fft_conv timings (profiling runs)")
    ap.add_argument("--tile", type=int, default=0, help="force the FFT tile length (0 = planner's choice)")
    ap.add_argument("--spinup-ms", type=float, default=80.0,
                    help="untimed device spin-up before the warm-up steps: the same launches, replayed for this long, so "
                         "that the timed steps see the clock the device holds in steady state, not its ramp from idle "
                         "(measured: 37.0 us per launch after 40 warm-up steps, 34.1 after 400, 33.4 after 2,000)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.tile:
        os.environ["FFTCONV_TILE"] = str(args.tile)
    # rehearsal knobs (single-GPU box): several ranks on one device, gloo instead of RCCL
    dev_index = int(os.environ.get("FFTCONV_BENCH_DEVICE", local_rank))
    backend = os.environ.get("FFTCONV_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import fft_conv_pytorch_amd as fca

    cfg = CONFIGS[args.config]
    ndim, batch, cin, cout, groups, spatial, kernel, dil = cfg
    total_batch = batch * world
    if args.scaling == "strong":
        # the node-level problem split over the ranks (no data-path collective: batch items are independent)
        from fft_conv_pytorch_amd.distributed import shard_range
        if args.config not in STRONG_BATCH:
            ap.error(f"--scaling strong needs one of {sorted(STRONG_BATCH)}")
        total_batch = STRONG_BATCH[args.config]
        lo, hi = shard_range(total_batch, world, rank)
        if hi == lo:
            ap.error(f"batch {total_batch} leaves rank {rank} of {world} without work")
        batch = hi - lo
        cfg = (ndim, batch, cin, cout, groups, spatial, kernel, dil)
    Layer = {1: fca.FFTConv1d, 2: fca.FFTConv2d, 3: fca.FFTConv3d}[ndim]
    torch.manual_seed(0)
    layer = Layer(cin, cout, kernel, dilation=dil, groups=groups, bias=True)
    with torch.no_grad():
        layer.weight.normal_()
        layer.bias.normal_()
    layer = layer.to(dev)
    if world > 1:   # every rank holds the same parameters (as after loading one checkpoint)
        dist.broadcast(layer.weight.data, src=0)
        dist.broadcast(layer.bias.data, src=0)
        layer.invalidate_kernel_spectrum()       # .data writes bypass the version counter the cache keys on
    layer.eval()                                  # inference: the module reuses the kernel spectrum per weight version

    # distinct buffer sets, > 2x the Infinity Cache in total
    in_bytes = 4 * batch * cin
    for s in spatial:
        in_bytes *= s
    nbuf = max(2, min(16, int(2.2 * 256 * 2**20 / (2 * in_bytes)) + 1))
    gen = torch.Generator(device=dev).manual_seed(1 + rank)
    xs = [torch.randn(batch, cin, *spatial, device=dev, generator=gen) for _ in range(nbuf)]
    with torch.no_grad():
        y0 = layer(xs[0])
    out_spatial = tuple(y0.shape[2:])
    ys = [torch.empty_like(y0) for _ in range(nbuf)]
    alg_bytes, n_out = algorithmic_bytes(batch, cin, cout, groups, spatial, kernel, out_spatial)

    spectrum = layer.__dict__["_spectrum_cache"][1]     # what the module's own forward uses
    plan = spectrum.plan
    if world > 1:
        # the path's only exchange: rank 0 transforms the kernel, RCCL broadcasts the spectrum over xGMI
        from fft_conv_pytorch_amd.distributed import broadcast_kernel_spectrum
        spectrum = broadcast_kernel_spectrum(plan, layer.weight.detach(), src=0)
    bias_ptr = layer.bias.data_ptr()
    stream = torch.cuda.current_stream(dev)
    from fft_conv_pytorch_amd.functional import new_workspace
    workspace = new_workspace(plan, dev)      # N-d plans only; the steps run one after another on one stream
    ws_ptr = workspace.data_ptr() if workspace is not None else None

    def step(i):
        j = i % nbuf
        plan.forward(xs[j].data_ptr(), spectrum.buf.data_ptr(), bias_ptr, ys[j].data_ptr(), ws_ptr,
                     torch.cuda.current_stream(dev).cuda_stream)

    steps, warmup = args.steps, args.warmup
    graph = None
    # launches per graph: whole rotations over the buffer sets, as many as the timed steps hold (at most 64 rotations),
    # so that K timed steps are a few replays plus at most nbuf - 1 eager launches whatever K is (a replay costs the host
    # 10-16 us: with one rotation per graph the driver's 20-step run paid two replays and two eager launches for 20 steps)
    per_graph = nbuf * max(1, min(64, steps // nbuf))
    if not args.no_graph:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            for i in range(nbuf):
                step(i)
        stream.wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(per_graph):
                step(i)

    def run(n):
        if graph is not None:
            for _ in range(n // per_graph):
                graph.replay()
            for i in range(n % per_graph):
                step(i)
        else:
            for i in range(n):
                step(i)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # device spin-up (untimed, not counted as steps): the clock takes tens of milliseconds of load to settle
    t_spin = time.perf_counter()
    while (time.perf_counter() - t_spin) * 1e3 < args.spinup_ms:
        run(max(4 * nbuf, per_graph))
        torch.cuda.synchronize(dev)
    run(warmup)
    fence()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    run(steps)
    ev1.record()
    fence()
    elapsed = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    if world > 1:
        t = torch.tensor([elapsed, dev_ms], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, dev_ms = float(t[0]), float(t[1])

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ys[(steps - 1) % nbuf])     # step i wrote ys[i % nbuf] (per_graph is a multiple of nbuf)

    if args.full:
        # light sanity check of the timed path's result (not a parity test: tests/ does that)
        assert torch.isfinite(ys[0]).all() and torch.allclose(ys[0], y0, rtol=0, atol=0)

    if rank == 0:
        out = {
            "metric": "GSamples/s (output elems/s), forward fft_conv",
            "value": (n_out // batch) * total_batch * steps / elapsed / 1e9,
            "unit": "GSamples/s",
            "n_gpus": world, "steps": steps, "warmup": warmup,
            "ms_per_step": elapsed * 1e3 / steps,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.config}: {ndim}D fft_conv B={batch}/GPU"
                                   f"{' (of ' + str(total_batch) + ' over the node)' if args.scaling == 'strong' else ''} {cin}->{cout}ch groups={groups} "
                                   f"spatial={list(spatial)} kernel={list(kernel)} dilation={dil} bias, fp32",
                       "tile": plan.tile, "buffer_sets": nbuf, "hip_graph": graph is not None, "launches_per_graph": per_graph if graph is not None else 0,
                       "spinup_ms": args.spinup_ms,
                       "kernel_spectrum": "cached per weight version (FFTConv module)"},
        }
        if args.full:
            kernel_us = dev_ms * 1e3 / steps          # HIP-event time per launch on the launch stream
            achieved = alg_bytes / (kernel_us * 1e-6) / 1e9
            step_us = elapsed * 1e6 / steps           # host clock around the same steps (what `value` is made of)
            out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                               "frac": achieved / HBM_PEAK_GBPS, "traffic": pmc_traffic(args.config, dominant_kernel_name(plan)),
                               "algorithmic_bytes_per_launch": alg_bytes, "kernel_us": kernel_us,
                               "kernel": dominant_kernel_name(plan),
                               "frac_from_ms_per_step": alg_bytes / (step_us * 1e-6) / 1e9 / HBM_PEAK_GBPS}
        if args.full and world == 1 and not args.no_end_to_end:
            # What a user's call costs end to end, launched eagerly from the host (no graph): the module with its
            # cached spectrum, and the functional fft_conv() that transforms the kernel on EVERY call like the
            # reference does (functional.py:71) and allocates its output -- the "uncached" figure of SURVEY 8d.
            from fft_conv_pytorch_amd.functional import fft_conv, transform_kernel
            with torch.no_grad():
                x0, wt, bs = xs[0], layer.weight.detach(), layer.bias.detach()
                kw = dict(dilation=dil, groups=groups)
                mod_dev, mod_wall = eager_us(lambda: layer(x0))
                unc_dev, unc_wall = eager_us(lambda: fft_conv(x0, wt, bs, **kw))
                tr_dev, _ = eager_us(lambda: transform_kernel(plan, wt))
            out["end_to_end"] = {
                "module_cached_us": mod_dev, "module_cached_host_us": mod_wall,
                "fft_conv_uncached_us": unc_dev, "fft_conv_uncached_host_us": unc_wall,
                "kernel_transform_us": tr_dev,
                "uncached_value": n_out / (max(unc_dev, unc_wall) * 1e-6) / 1e9, "unit": "us / GSamples/s",
                "note": "eager launches, input re-read from cache (one buffer); uncached = kernel transform + forward + output allocation per call"}
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
