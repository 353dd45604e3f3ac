#!/usr/bin/env python3
"""What the 1-D planner decides, one JSON line per (descriptor, knob setting): plans are created and destroyed, nothing
is launched.  Two builds of the library plan alike exactly when their outputs are byte-identical:

    FFTCONV_LIB=/path/to/one/libfftconv_amd.so   python scripts/route_dump.py --out a.jsonl
    FFTCONV_LIB=/path/to/other/libfftconv_amd.so python scripts/route_dump.py --out b.jsonl
    cmp a.jsonl b.jsonl && sha256sum a.jsonl

A line holds the status of fc_plan_create (and the error text of a failure), the words of fc_debug_route and
fc_plan_layout, the tile, spectrum and workspace bytes, the output shape, fc_debug_grid, and fc_wgrad1d_slices /
fc_wgrad1d_db_supported of the same descriptor.

Inputs: every float32 1-D case of tests/route_util.py (ROUTES, which holds TAIL_SPLIT_CASES) under its own knobs, then a
seeded sweep of descriptors, each under every state of KNOB_STATES.  The sweep keeps batch x tiles small enough that no
work list passes MAX_ITEMS items."""
import argparse
import ctypes
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fft_conv_pytorch_amd import _native  # noqa: E402

KNOBS = ("FFTCONV_PERS", "FFTCONV_PH2", "FFTCONV_DENSE", "FFTCONV_WIDE", "FFTCONV_DIAG", "FFTCONV_DENSE_SLAB")
KNOB_STATES = ([{}] + [{"FFTCONV_PERS": v} for v in "0124"] + [{"FFTCONV_PH2": v} for v in "01"] +
               [{"FFTCONV_DENSE": v} for v in "02"] + [{"FFTCONV_WIDE": "0"}, {"FFTCONV_DIAG": "0"}])
MAX_ITEMS = 1_000_000
F32, F16 = 0, 2


def items_bound(B, cout, L, K, s, p, d, tr, op, hint):
    """Upper bound of the work-list length of any plan of the descriptor: virtual batch x tiles x out-chunks, over the
    tiles the batch-sharing kernels have (or the hinted one) and the kernel extents a tile may be planned for."""
    kd = (K - 1) * d + 1
    Lf = (L - 1) * s - 2 * p + kd + op if tr else L + 2 * p - kd + 1
    if Lf < 1:
        return 0
    seg = (min(max(1, 1024 // d + 1), K) - 1) * d + 1
    worst = 0
    for T in {1024, 2048, hint} - {0}:
        for ext in (kd, K, seg):
            if T >= ext:
                worst = max(worst, B * (Lf // (T - ext + 1) + d + 1) * max(1, -(-cout // 8)))
    return worst


def sweep(n, seed):
    """n descriptors as keyword arguments of _native.conv_desc."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        kind = rng.choice(("dense", "dense", "dense", "depthwise", "blocks", "no-blocks"))
        if kind == "dense":
            g = rng.choice((1, 1, 1, 2, 3))
            cin, cout = g * rng.randint(1, 64), g * rng.randint(1, 64)
            if rng.random() < 0.3:      # whole 8-blocks: the batch-sharing shapes
                cin, cout = g * rng.choice((8, 16, 24, 32, 64)), g * rng.choice((8, 16, 24, 32, 64))
        elif kind == "depthwise":
            g = rng.choice((5, 7, 8, 16, 24))
            cin = cout = g
        else:
            gs = rng.choice((2, 4))
            per_block = 8 // gs
            g = per_block * rng.randint(1, 4) if kind == "blocks" else per_block * rng.randint(0, 3) + rng.randint(1, per_block - 1)
            cin = cout = g * gs
        batches = (1, 2, 3, 4, 5, 8, 32, 64)
        B = rng.choice(batches)
        L = int(2 ** rng.uniform(6, 20))
        if rng.random() < 0.15:
            L = 1 << rng.randint(6, 20)
        K = max(1, min(6000, int(2 ** rng.uniform(0, 12.56))))
        s = rng.choice((1, 1, 1, 1, 2, 3))
        d = rng.choice((1, 1, 1, 2, 3, 4, 5, 6, 7, 8))
        tr = rng.random() < 0.15
        mode = 0 if tr else rng.randrange(4)
        hint = rng.choice((0, 0, 0, 0, 256, 1024, 2048, 4096))
        dtype = F16 if rng.random() < 0.2 else F32
        if (K - 1) * d + 1 > L and rng.random() < 0.9:      # mostly kernels that fit the row
            K = max(1, (L - 1) // d + 1)
        kd = (K - 1) * d + 1
        p = rng.choice((0, (kd - 1) // 2, kd - 1, rng.randint(0, 40)))
        if mode in (1, 3):
            p = min(p, L - 1)
        if tr:
            p = min(p, kd - 1)
        op = rng.randint(0, s - 1) if tr else 0
        while items_bound(B, cout, L, K, s, p, d, tr, op, hint) > MAX_ITEMS:
            if B > 1 and rng.random() < 0.5:
                B = batches[batches.index(B) - 1]
            else:
                L = max(64, L // 2)
                if L == 64 and B == 1:
                    K = max(1, K // 2)
                p = min(p, L - 1, (K - 1) * d if tr else p)
        out.append(dict(ndim=1, batch=B, cin=cin, cout=cout, groups=g, spatial=(L,), kernel=(K,), stride=(s,), padding=(p,),
                        dilation=(d,), mode=mode, dtype=dtype, has_bias=rng.random() < 0.5, tile_hint=hint, transposed=tr,
                        output_padding=(op,)))
    return out


def route_cases():
    """(descriptor, knobs) of every float32 1-D case of tests/route_util.py, under the route's and its own knobs."""
    from tests import route_util as ru
    out = []
    for route in ru.ROUTES:
        for c in route.cases:
            if c.nd != 1 or c.f64:
                continue
            env = {k: v for k, v in {**route.env, **c.env}.items() if v is not None}
            hint = int(env.pop("FFTCONV_TILE", "0"))
            out.append((dict(ndim=1, batch=c.B, cin=c.cin, cout=c.cout, groups=c.g, spatial=c.size, kernel=c.k,
                             stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), mode=_native.PAD_MODES[c.mode],
                             dtype=F32, has_bias=True, tile_hint=hint, transposed=c.tr, output_padding=c.tup(c.op)), env))
    return out


def describe(lib, kw, env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    desc = _native.conv_desc(**kw)
    rec = {"desc": {k: (list(v) if isinstance(v, tuple) else int(v)) for k, v in kw.items()}, "env": env}
    handle = ctypes.c_void_p()
    rec["status"] = int(lib.fc_plan_create(ctypes.byref(desc), ctypes.byref(handle)))
    if rec["status"] != _native.FC_OK:
        rec["error"] = lib.fc_last_error().decode("utf-8", "replace")
    else:
        words, lay, shape = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 8)(), (ctypes.c_int64 * 3)()
        _native._check(lib, lib.fc_debug_route(handle, ctypes.byref(words)))
        _native._check(lib, lib.fc_plan_layout(handle, ctypes.byref(lay)))
        _native._check(lib, lib.fc_output_shape(handle, ctypes.byref(shape)))
        rec.update(route=list(words), layout=list(lay), tile=int(lib.fc_plan_tile(handle)),
                   spectrum_bytes=int(lib.fc_kernel_spectrum_bytes(handle)),
                   workspace_bytes=int(lib.fc_workspace_bytes(handle)), out=list(shape),
                   grid=int(lib.fc_debug_grid(handle)))
        assert rec["route"][15] <= MAX_ITEMS, rec       # (f32_1d: word 15 is pers_items)
        lib.fc_plan_destroy(handle)
    rec["wgrad1d_slices"] = int(lib.fc_wgrad1d_slices(ctypes.byref(desc)))
    rec["wgrad1d_db_supported"] = int(lib.fc_wgrad1d_db_supported(ctypes.byref(desc)))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=2000, help="descriptors of the seeded sweep")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()
    import torch
    torch.cuda.init()          # (the library plans for the current HIP device)
    lib = _native.load_library()
    runs = route_cases() + [(kw, env) for kw in sweep(args.n, args.seed) for env in KNOB_STATES]
    n_ok = n_sharing = 0
    with open(args.out, "w") as f:
        for kw, env in runs:
            rec = describe(lib, kw, env)
            n_ok += rec["status"] == _native.FC_OK
            n_sharing += rec["status"] == _native.FC_OK and rec["route"][3] != 0
            f.write(json.dumps(rec, sort_keys=True) + "\n")
    print(f"{len(runs)} lines, {n_ok} plans, {n_sharing} of them with a work list -> {args.out}")


if __name__ == "__main__":
    main()
