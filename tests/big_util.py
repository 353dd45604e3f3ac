"""Exact truth for tensors of several GiB at no cost (tests/test_gpu_thresholds.py; tests/test_host_big_util.py runs all of
it on the CPU).

Sparse inputs.  x (and dY) is zero except in windows of WIN small integers (accuracy_util.integers: exact in float32, float16
and bfloat16), every window with values of its own, so that a read that wraps to ``offset mod 2**32`` or ``mod 2**31`` finds
another number, not the right one by luck.  ``windows`` places them, for a tensor (B, C, *spatial) whose rows are its last
axis: at the start, at the start of the last tile and at the end of every row it touches; in the first and last row of the
tensor (in every row of a tensor of at most ALL_ROWS rows, in the first and last row of every channel of a tensor of at most
ALL_ROWS channels); on both sides of every multiple of ``step`` bytes (2**30) counted from the tensor base, from every
batch-item base and from every group base; and ``reach`` samples from both row ends, where the first and the last tap of a
kernel of that extent meet the ends of the row.  ``step`` is a parameter: the host test scales the crossings down to 4096 bytes.

Truth.  ``conv_truth`` is the float64 scatter of (nonzero sample) x (tap) products over everything a route_util.Case carries:
forward and transposed, stride, padding, dilation, groups, the four padding modes, 1-D to 3-D.  ``wgrad_truth`` is the same
from two sparse tensors.  Both return a COO list (flat index, value); nothing dense is ever built.  All values are integers
far below 2**53, so the sums are exact in any order.

Check.  ``check_full`` compares EVERY sample of an output with the truth (bias + scattered list), on the output's device in
chunks of CHUNK_BYTES of float64: max|got - want| <= tol * max|want| and no NaN, so an output allocated under
guard_util.guarded_empty(0xFF) also shows every sample the kernels never stored.  A 16-bit output is compared with the
float32 truth rounded once."""
import itertools
import math

import numpy as np
import torch

from tests import accuracy_util as au

WIN = 4
STEP = 1 << 30
CHUNK_BYTES = 256 << 20
ALL_ROWS = 64            # at most this many rows: windows in every row; channels: in the first and last row of each


class Sparse:
    """A tensor given by its nonzero samples: ``flat`` (sorted, unique flat indices) and ``val`` (float64)."""

    def __init__(self, shape, flat, val):
        self.shape = tuple(int(s) for s in shape)
        flat = np.asarray(flat, dtype=np.int64)
        val = np.asarray(val, dtype=np.float64)
        flat, first = np.unique(flat, return_index=True)
        self.flat, self.val = flat, val[first]
        assert flat.size == 0 or (flat[0] >= 0 and flat[-1] < math.prod(self.shape))

    @classmethod
    def from_dense(cls, t):
        a = t.detach().cpu().double().numpy().reshape(-1)
        nz = np.nonzero(a)[0]
        return cls(t.shape, nz, a[nz])

    def coords(self):
        return np.stack(np.unravel_index(self.flat, self.shape), 1).astype(np.int64)

    def dense(self, dtype, device="cpu"):
        """zeros plus a scatter of the samples"""
        t = torch.zeros(self.shape, dtype=dtype, device=device)
        t.view(-1)[torch.from_numpy(self.flat).to(device)] = torch.from_numpy(self.val).to(dtype).to(device)
        return t


# ------------------------------------------------------------------------------------------------ window placement
def crossings(shape, itemsize, groups=1, step=STEP):
    """Flat element indices e at which a multiple of ``step`` bytes, counted from the tensor base, from a batch-item base
    or from a group base, falls inside the tensor (sorted, unique)."""
    B, C = shape[0], shape[1]
    S = math.prod(shape[2:])
    total = B * C * S
    assert step % itemsize == 0
    se = step // itemsize
    bases = {0}
    for b in range(B):
        bases.update((b * groups + g) * (C // groups) * S for g in range(groups))
    out = set()
    for base in bases:
        out.update(range(base + se, total, se))
    return sorted(out)


def windows(shape, itemsize, groups=1, tile=1024, reach=1, step=STEP, win=WIN):
    """Sorted list of (flat start, length) of the windows of a tensor (B, C, *spatial); see the module docstring."""
    L = shape[-1]
    total = math.prod(shape)
    nrows = total // L
    runs = set()

    def add(lo, n):
        lo, hi = max(lo, 0), min(lo + n, total)
        if hi > lo:
            runs.add((lo, hi - lo))

    rows = set(range(nrows)) if nrows <= ALL_ROWS else {0, nrows - 1}
    per_channel = math.prod(shape[2:-1])
    if shape[0] * shape[1] <= ALL_ROWS:          # the first and the last row of every channel: no row base goes unread
        for ch in range(shape[0] * shape[1]):
            rows.update({ch * per_channel, (ch + 1) * per_channel - 1})
    for e in crossings(shape, itemsize, groups, step):
        add(e - win, win)
        add(e, win)
        rows.update({(e - 1) // L, e // L})
    for r in rows:
        last_tile = (L - 1) // tile * tile
        for pos in (0, last_tile, L - win, reach - 1, L - reach - win + 1):
            pos = min(max(pos, 0), max(L - win, 0))
            add(r * L + pos, min(win, L))
    return sorted(runs)


def sparse_input(shape, itemsize, seed, groups=1, tile=1024, reach=1, step=STEP, win=WIN):
    """The Sparse tensor of ``windows``: integers of accuracy_util's centred class, a zero drawn becomes HI (a window
    sample that reads as zero would say nothing)."""
    runs = windows(shape, itemsize, groups, tile, reach, step, win)
    flat = np.concatenate([np.arange(lo, lo + n) for lo, n in runs])
    vals = au.integers((flat.size,), torch.Generator().manual_seed(seed), torch.float64).numpy().copy()
    vals[vals == 0] = au.HI
    return Sparse(shape, flat, vals)


# ------------------------------------------------------------------------------------------------ truth
def _padded_sources(L, p, mode):
    """source position -> padded positions q in [0, L + 2p) of the BORDER that read it (the interior is q = pos + p)"""
    if mode == "constant" or p == 0:
        return {}
    q = np.concatenate([np.arange(0, p), np.arange(L + p, L + 2 * p)])
    r = q - p
    if mode == "reflect":
        src = np.where(r < 0, -r, 2 * (L - 1) - r)
    elif mode == "replicate":
        src = np.clip(r, 0, L - 1)
    elif mode == "circular":
        src = np.mod(r, L)
    else:
        raise ValueError(mode)
    table = {}
    for qi, si in zip(q.tolist(), src.tolist()):
        table.setdefault(si, []).append(qi)
    return table


def _expand_padded(c, xs):
    """The samples of xs as samples of the padded signal: (batch, channel, padded coords (n, nd), value)."""
    co = xs.coords()
    pads = c.tup(c.p)
    if c.tr or c.mode == "constant":
        return co[:, 0], co[:, 1], co[:, 2:] + (0 if c.tr else np.asarray(pads)), xs.val
    tables = [_padded_sources(c.size[a], pads[a], c.mode) for a in range(c.nd)]
    rows, vals = [], []
    for row, v in zip(co.tolist(), xs.val.tolist()):
        per_axis = [[row[2 + a] + pads[a]] + tables[a].get(row[2 + a], []) for a in range(c.nd)]
        for q in itertools.product(*per_axis):
            rows.append(row[:2] + list(q))
            vals.append(v)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2 + c.nd)
    return rows[:, 0], rows[:, 1], rows[:, 2:], np.asarray(vals, dtype=np.float64)


def _coalesce(flat, val):
    if flat.size == 0:
        return flat.astype(np.int64), val.astype(np.float64)
    u, inv = np.unique(flat, return_inverse=True)
    return u, np.bincount(inv.reshape(-1), weights=val, minlength=u.size)


def conv_truth(c, xs, w, max_terms=1 << 24):
    """COO list (flat index into (B, Cout, *out), float64 value) of the convolution of route_util.Case ``c`` applied to
    the Sparse signal ``xs`` with the dense weight ``w`` (numpy, c.wshape), without the bias."""
    nd, out = c.nd, au.out_spatial(c)
    s, d, p = (np.asarray(c.tup(v)) for v in (c.s, c.d, c.p))
    cig, cog = c.cin // c.g, c.cout // c.g
    b, ci, q, val = _expand_padded(c, xs)
    taps = np.stack(np.unravel_index(np.arange(math.prod(c.k)), c.k), 1).astype(np.int64)     # (K, nd)
    outv = np.asarray(out)
    flats, vals = [], []
    per = max(1, max_terms // (taps.shape[0] * cog))
    for lo in range(0, b.size, per):
        sl = slice(lo, lo + per)
        if c.tr:
            o = q[sl, None, :] * s - p + taps[None] * d
            ok = ((o >= 0) & (o < outv)).all(2)
        else:
            num = q[sl, None, :] - taps[None] * d
            o = num // s
            ok = ((num >= 0) & (num % s == 0) & (o < outv)).all(2)
        si, ti = np.nonzero(ok)
        if si.size == 0:
            continue
        oo = np.ravel_multi_index(tuple(o[si, ti].T), out)
        bb, cc, vv = b[sl][si], ci[sl][si], val[sl][si]
        g, cin_g = cc // cig, cc % cig
        tk = tuple(taps[ti].T)
        for j in range(cog):
            wv = w[(cc, np.full_like(cc, j)) + tk] if c.tr else w[(g * cog + j, cin_g) + tk]
            flats.append((bb * c.cout + g * cog + j) * math.prod(out) + oo)
            vals.append(vv * wv.astype(np.float64))
    if not flats:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    return _coalesce(np.concatenate(flats), np.concatenate(vals))


def wgrad_truth(c, xs, dys):
    """COO list over the weight (Cout, Cin/g, *k) of the weight gradient of the forward Case ``c`` from the Sparse signal
    and the Sparse output gradient: dW[o][i][k] = sum_b sum_t dY[b][o][t] Xp[b][i][t s + k d]."""
    assert not c.tr
    s, d = (np.asarray(c.tup(v)) for v in (c.s, c.d))
    cig, cog = c.cin // c.g, c.cout // c.g
    kv = np.asarray(c.k)
    xb, xc, xq, xv = _expand_padded(c, xs)
    yco = dys.coords()
    flats, vals = [], []
    for b in np.intersect1d(xb, yco[:, 0]).tolist():
        ix, iy = np.nonzero(xb == b)[0], np.nonzero(yco[:, 0] == b)[0]
        num = xq[ix][:, None, :] - yco[iy][None, :, 2:] * s                     # (nx, ny, nd) = k d
        k = num // d
        ok = ((num >= 0) & (num % d == 0) & (k < kv)).all(2) & ((xc[ix] // cig)[:, None] == (yco[iy, 1] // cog)[None, :])
        i, j = np.nonzero(ok)
        kk = np.ravel_multi_index(tuple(k[i, j].T), c.k)
        flats.append((yco[iy[j], 1] * cig + xc[ix[i]] % cig) * math.prod(c.k) + kk)
        vals.append(xv[ix[i]] * dys.val[iy[j]])
    if not flats:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    return _coalesce(np.concatenate(flats), np.concatenate(vals))


def bias_grad_truth(dys):
    """db (Cout,) of a Sparse output gradient"""
    return np.bincount(dys.coords()[:, 1], weights=dys.val, minlength=dys.shape[1])


# ------------------------------------------------------------------------------------------------ check
def check_full(got, flat, val, bias=None, tol=1e-4, chunk_bytes=CHUNK_BYTES, what="output"):
    """Every sample of ``got`` (B, C, *spatial), contiguous, against bias[c] + the COO list: raises AssertionError on a
    NaN or when max|got - want| > tol * max|want|; returns (max|got - want|, max|want|).  Chunks of chunk_bytes of float64
    on got's device."""
    assert got.is_contiguous()
    dev, total = got.device, got.numel()
    C, S = got.shape[1], math.prod(got.shape[2:])
    gflat = got.view(-1)
    bias64 = None if bias is None else torch.as_tensor(np.asarray(bias, dtype=np.float64), device=dev)
    order = np.argsort(flat, kind="stable")
    flat, val = np.asarray(flat)[order], np.asarray(val, dtype=np.float64)[order]
    n = max(1, chunk_bytes // 8)
    step = n // S * S if S <= n else n          # whole rows where a row fits, else pieces of one row
    worst, wmax, where = 0.0, 0.0, -1
    pos = 0
    while pos < total:
        hi = min(pos + step, total) if S <= n else min(pos + step, (pos // S + 1) * S)
        want = torch.zeros(hi - pos, dtype=torch.float64, device=dev)
        if bias64 is not None:
            if S <= n:
                rows = torch.arange(pos // S, hi // S, device=dev) % C
                want.view(-1, S).add_(bias64[rows][:, None])
            else:
                want.add_(bias64[(pos // S) % C])
        a, b = np.searchsorted(flat, pos), np.searchsorted(flat, hi)
        if b > a:
            want.index_add_(0, torch.from_numpy(flat[a:b] - pos).to(dev), torch.from_numpy(val[a:b]).to(dev))
        if got.dtype in (torch.float16, torch.bfloat16):
            want = want.float().to(got.dtype).double()           # the float32 result rounded once
        wmax = max(wmax, want.abs().max().item())
        diff = (gflat[pos:hi].double() - want).abs_()
        m = diff.max().item()
        if math.isnan(m):
            bad = torch.isnan(diff)
            first = pos + int(bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} samples of flat [{pos}, {hi}) are NaN (never written?), the first "
                                 f"at {np.unravel_index(first, tuple(got.shape))}")
        if m > worst:
            worst, where = m, pos + int(diff.argmax())
        pos = hi
    assert worst <= tol * wmax, (f"{what}: max|got - want| = {worst:.3e} at {np.unravel_index(where, tuple(got.shape))} > "
                                 f"{tol} x max|want| = {tol * wmax:.3e}")
    return worst, wmax
