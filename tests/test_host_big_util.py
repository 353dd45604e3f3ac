"""tests/big_util.py on the CPU: the sparse truth equals torch's float64 convolutions and autograd's dW; the full check
catches the faults it is for, on numpy models of a kernel with the 2**30 / 2**31 / 2**32 crossings scaled down to 4096
bytes; the window list holds both sides of every crossing."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import accuracy_util as au
from tests import big_util as bu
from tests import route_util as ru

C = ru.Case
TRUTH_CASES = [
    C(2, 4, 6, (50,), (5,), p=2),
    C(2, 4, 6, (50,), (5,), s=2, p=3, d=2, g=2, mode="reflect"),
    C(3, 6, 3, (41,), (4,), s=3, p=4, g=3, mode="replicate"),
    C(2, 2, 2, (30,), (7,), p=30, d=3, mode="circular"),
    C(2, 4, 6, (20,), (5,), s=2, p=1, op=1, d=2, g=2, tr=True),
    C(1, 3, 2, (12,), (3,), s=3, p=0, op=2, tr=True),
    C(2, 4, 4, (9, 11), (3, 2), s=(1, 2), p=(2, 1), d=(2, 1), g=2, mode="reflect"),
    C(1, 2, 3, (8, 7), (3, 3), p=(1, 2), mode="circular"),
    C(2, 2, 2, (6, 9), (2, 3), s=2, p=(1, 0), mode="replicate"),
    C(2, 4, 2, (5, 6), (3, 2), s=(2, 3), p=(1, 0), op=(1, 2), g=2, tr=True),
    C(1, 2, 4, (5, 6, 7), (2, 3, 2), s=(1, 2, 1), p=1, d=(2, 1, 1), g=2),
    C(1, 2, 2, (4, 5, 6), (2, 2, 3), p=(1, 2, 1), mode="reflect"),
    C(1, 2, 2, (3, 4, 3), (2, 3, 2), s=2, p=1, op=1, d=(1, 1, 2), tr=True),
]


def _reference(c, x, w, b):
    if c.tr:
        fn = (F.conv_transpose1d, F.conv_transpose2d, F.conv_transpose3d)[c.nd - 1]
        return fn(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), groups=c.g, dilation=c.tup(c.d))
    conv = (F.conv1d, F.conv2d, F.conv3d)[c.nd - 1]
    flat = [q for p in reversed(c.tup(c.p)) for q in (p, p)]
    xp = F.pad(x, flat, mode=c.mode) if c.mode != "constant" else F.pad(x, flat)
    return conv(xp, w, b, stride=c.tup(c.s), dilation=c.tup(c.d), groups=c.g)


def _sparse_dense(shape, seed, keep=0.3):
    gen = torch.Generator().manual_seed(seed)
    t = au.integers(shape, gen, torch.float64)
    return t * (torch.rand(shape, generator=gen) < keep)


@pytest.mark.parametrize("c", TRUTH_CASES, ids=[c.ident() for c in TRUTH_CASES])
def test_truth_equals_torch(c):
    x = _sparse_dense((c.B, c.cin) + tuple(c.size), 1)
    w = au.integers(c.wshape, torch.Generator().manual_seed(2), torch.float64)
    b = au.integers((c.cout,), torch.Generator().manual_seed(3), torch.float64)
    want = _reference(c, x, w, b)
    assert tuple(want.shape[2:]) == au.out_spatial(c)
    flat, val = bu.conv_truth(c, bu.Sparse.from_dense(x), w.numpy())
    worst, wmax = bu.check_full(want, flat, val, b.numpy(), tol=0.0, chunk_bytes=8 * 100)
    assert worst == 0.0 and wmax > 0
    # (split into several rounds of samples: the same list)
    flat2, val2 = bu.conv_truth(c, bu.Sparse.from_dense(x), w.numpy(), max_terms=1)
    assert np.array_equal(flat, flat2) and np.array_equal(val, val2)


@pytest.mark.parametrize("c", [c for c in TRUTH_CASES if not c.tr], ids=[c.ident() for c in TRUTH_CASES if not c.tr])
def test_wgrad_truth_equals_autograd(c):
    x = _sparse_dense((c.B, c.cin) + tuple(c.size), 4)
    w = au.integers(c.wshape, torch.Generator().manual_seed(5), torch.float64).requires_grad_()
    b = torch.zeros(c.cout, dtype=torch.float64, requires_grad=True)
    y = _reference(c, x, w, b)
    dy = _sparse_dense(tuple(y.shape), 6)
    y.backward(dy)
    flat, val = bu.wgrad_truth(c, bu.Sparse.from_dense(x), bu.Sparse.from_dense(dy))
    assert bu.check_full(w.grad[None], flat, val, None, tol=0.0)[0] == 0.0
    assert np.array_equal(bu.bias_grad_truth(bu.Sparse.from_dense(dy)), b.grad.numpy())


def test_check_full_reports_nan_and_errors():
    got = torch.zeros(2, 3, 50)
    got[1, 2, 7] = 5.0
    flat = np.array([(1 * 3 + 2) * 50 + 7])
    for chunk in (8 * 20, 8 * 50, 8 * 120, 1 << 20):       # pieces of a row, one row, two rows, everything
        assert bu.check_full(got, flat, np.array([5.0]), chunk_bytes=chunk) == (0.0, 5.0)
        with pytest.raises(AssertionError, match="max.got - want"):
            bu.check_full(got, flat, np.array([5.01]), chunk_bytes=chunk)
        bad = got.clone()
        bad[0, 1, 49] = float("nan")
        with pytest.raises(AssertionError, match="NaN"):
            bu.check_full(bad, flat, np.array([5.0]), chunk_bytes=chunk)
    half = got.to(torch.bfloat16)
    half[1, 2, 7] = 5.03125                      # 5.04 rounded once to bfloat16
    bu.check_full(half, flat, np.array([5.04]), tol=0.0)


# ------------------------------------------------------------------------------------------------ window placement
def test_windows_hold_both_sides_of_every_crossing():
    shape, item, groups, step = (3, 4, 1500), 4, 2, 4096
    runs = bu.windows(shape, item, groups, tile=448, reach=33, step=step)
    cover = np.zeros(math.prod(shape), dtype=bool)
    for lo, n in runs:
        cover[lo:lo + n] = True
    cross = bu.crossings(shape, item, groups, step)
    S = 4 * 1500
    expect = {base + m * 1024 for base in [0] + [b * S for b in range(3)] + [b * S + 3000 for b in range(3)]
              for m in range(1, 20) if base + m * 1024 < 3 * S}
    assert set(cross) == expect
    for e in cross:
        assert cover[e - 1] and cover[e], e
    for r in (0, 11) + tuple(e // 1500 for e in cross):
        row = cover[r * 1500:(r + 1) * 1500]
        assert row[0] and row[-1] and row[1344] and row[32] and row[1500 - 33], r
    assert bu.windows(shape, item, groups, tile=448, reach=33, step=step) == runs            # pure
    xs = bu.sparse_input(shape, item, 1, groups, tile=448, reach=33, step=step)
    assert np.array_equal(np.nonzero(cover)[0], xs.flat) and (xs.val != 0).all()
    # no window repeats another: a wrapped read finds other numbers
    vals = [tuple(xs.val[np.searchsorted(xs.flat, lo):np.searchsorted(xs.flat, lo) + n]) for lo, n in runs if n == bu.WIN]
    assert len(set(vals)) > 0.9 * len(vals)


# ------------------------------------------------------------------------------------------------ the faults it is for
STEP = 4096                 # stands for 2**30 bytes: "2**31" is 2 * STEP, "2**32" is 4 * STEP


def model_conv1d(x, w, b, p, V, cob, fault=None):
    """numpy model of a 1-D stride-1 zero-padded kernel as the HIP ones address memory: x read through a resource over one
    batch item's rows with 32-bit byte offsets, y stored tile by tile (V outputs, lanes past the row marked dead by the top
    bit of their offset) through a resource over ``cob`` output rows.  Faults, with the byte limits scaled to STEP:
    "wrap"     x offsets taken modulo 4 * STEP (a row base computed in 32 bits);
    "dead"     the dead bit is bit "31" = 2 * STEP: a dead store lands inside a row block longer than that;
    "truncate" the x resource's size is taken modulo 4 * STEP: loads past it return zero."""
    B, cin, L = x.shape
    cout, _, K = w.shape
    Lout = L + 2 * p - K + 1
    y = np.full((B, cout, Lout), np.nan)
    xf = x.reshape(-1)
    xbytes = cin * L * 4
    size = xbytes % (4 * STEP) if fault == "truncate" else xbytes
    dead_bit = 2 * STEP
    for bi in range(B):
        def load(ci, pos):
            if pos < 0 or pos >= L:
                return 0.0
            off = (ci * L + pos) * 4
            if off + 4 > size:
                return 0.0
            e = bi * cin * L + off // 4
            if fault == "wrap":
                e = (e * 4 % (4 * STEP)) // 4
            return xf[e]
        for c0 in range(0, cout, cob):
            block = y[bi, c0:c0 + cob].reshape(-1)         # the resource: cob rows
            for t0 in range(0, Lout, V):
                for n in range(V):
                    for r in range(min(cob, cout - c0)):
                        o = t0 + n
                        live = o < Lout
                        v = b[c0 + r] + (sum(w[c0 + r, ci, k] * load(ci, o - p + k) for ci in range(cin) for k in range(K))
                                         if live else 1000.0 + n)
                        off = (r * Lout + o) * 4
                        if not live:
                            off |= dead_bit if fault == "dead" else 1 << 62
                        if off + 4 <= block.size * 4:
                            block[off // 4] = v
            y[bi, c0:c0 + cob] = block.reshape(-1, Lout)
    return y


@pytest.fixture(scope="module")
def model_case():
    c = C(2, 2, 4, (1300,), (3,), p=1)            # x: 10400 bytes per batch item, y: 4 rows of 5200 bytes per block
    xs = bu.sparse_input((c.B, c.cin) + c.size, 4, 7, tile=64, reach=3, step=STEP)
    w = au.integers(c.wshape, torch.Generator().manual_seed(8), torch.float64).numpy()
    b = np.arange(1.0, c.cout + 1)
    flat, val = bu.conv_truth(c, xs, w)
    return c, xs.dense(torch.float64).numpy(), w, b, flat, val


def test_model_without_a_fault_passes(model_case):
    c, x, w, b, flat, val = model_case
    y = model_conv1d(x, w, b, 1, 64, 4)
    assert bu.check_full(torch.from_numpy(y), flat, val, b, tol=0.0, chunk_bytes=8 * 3000)[0] == 0.0


@pytest.mark.parametrize("fault", ["wrap", "dead", "truncate"])
def test_check_catches_the_fault(model_case, fault):
    c, x, w, b, flat, val = model_case
    # (x is 20800 bytes, past 4 STEP; a block of 4 y rows is 20800 bytes, past 2 STEP; a batch item of x is 10400 bytes,
    # below 4 STEP, so the truncation case takes 9 channels instead)
    if fault == "truncate":
        c = C(1, 9, 4, (1300,), (3,), p=1)        # 46800 bytes per batch item -> 46800 mod 16384 = 14032
        xs = bu.sparse_input((c.B, c.cin) + c.size, 4, 7, tile=64, reach=3, step=STEP)
        w = au.integers(c.wshape, torch.Generator().manual_seed(8), torch.float64).numpy()
        flat, val = bu.conv_truth(c, xs, w)
        x = xs.dense(torch.float64).numpy()
        assert bu.check_full(torch.from_numpy(model_conv1d(x, w, b, 1, 64, 4)), flat, val, b, tol=0.0)[0] == 0.0
    y = model_conv1d(x, w, b, 1, 64, 4, fault=fault)
    with pytest.raises(AssertionError):
        bu.check_full(torch.from_numpy(y), flat, val, b, tol=1e-4, chunk_bytes=8 * 3000)
