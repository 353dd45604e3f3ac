"""The conditions the case table of tests/long_sweep_util.py must meet, checked on the CPU: every pair of axis values the
API allows together occurs, the routes the library predicts under each case's switches meet their quotas (and the record's
own route, N1 x N2 and slab count are the library's), the truth of every case is exact, the checker of the GPU run rejects
each fault model on every case where the defect changes a value and accepts the float32 baseline, and the table does not
depend on the process that builds it."""
import collections
import dataclasses
import hashlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import long_sweep_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 9


def _all():
    fwd, tr = su.tables()
    return fwd + tr


def _switch(monkeypatch, c):
    su.set_switches(c, lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v))


def test_table_sizes_and_what_each_case_does():
    fwd, tr = su.tables()
    assert 48 <= len(fwd) <= 64 and 24 <= len(tr) <= 48, (len(fwd), len(tr))
    assert len({c.id for c in fwd + tr}) == len(fwd) + len(tr)
    for cases in (fwd, tr):
        for i, c in enumerate(cases):
            assert c.idx == i and c.grads == (i % 2 == 0) and c.module == (i % 8 in (0, 5)), c.id
            assert (c.cls == "offset") == (i % 3 == 0) and (c.dy == "none") == (not c.grads), c.id
            assert su.ROW["short"][0] <= c.rowlen <= 16384 and dict(c.pick)["row"] == \
                next(k for k, (lo, hi) in su.ROW.items() if lo <= c.rowlen <= hi), c.id
            assert c.rowlen > 4096 or c.route == "handoff" or c.complex, c.id
            assert c.cout % c.groups == 0 and (dict(c.pick)["groups"] != "dw" or (c.groups == c.cin and c.cig == 1)), c.id
    assert any(c.causal and c.K >= c.L for c in fwd) and any(c.K <= 17 for c in fwd)
    assert any(c.cout % 4 for c in fwd) and any(c.cout % 2 for c in fwd)      # not a multiple of any out_block


def test_every_allowed_pair_of_axis_values_occurs():
    for kind, cases in zip(("fwd", "tr"), su.tables()):
        covered = set()
        for c in cases:
            covered |= su.pairs_of(c)
        missing = sorted((q for q in su.allowed_pairs(kind) if q not in covered), key=repr)
        assert not missing, f"{kind}: {len(missing)} allowed pairs occur in no case, e.g. {missing[:8]}"


def _why_refused(kind, a, va, b, vb):
    """The rule that refuses two axis values together, or None."""
    d = {a: va, b: vb}
    has = lambda **kw: all(k in d and (d[k] in v if isinstance(v, tuple) else d[k] == v) for k, v in kw.items())  # noqa: E731
    if has(groups="dw", cig=(2, 3)):
        return "depthwise means groups = Cin, one input channel per group"
    if has(grads=True, dy="none") or has(grads=False, dy=("ncl", "nlc")):
        return "dY lies somewhere exactly when gradients are taken"
    if kind == "fwd":
        if has(padding="same", stride=(2, 3, 7)):
            return "ValueError: padding='same' is not supported for strided convolutions"
        if has(causal=True, padding=("odd", "same", "valid", "max")):
            return "ValueError: causal=True pads the row itself, padding must be 0"
        if has(causal=True, mode=("reflect", "replicate", "circular")):
            return "ValueError: causal=True pads with zeros, padding_mode must be 'constant'"
        if has(kclass="row", causal=False):
            return "ValueError: a kernel longer than the padded row (K >= L is the causal form's)"
        if has(kclass="row", padding=("odd", "same", "valid", "max")) or has(kclass="row", mode=("reflect", "replicate", "circular")):
            return "K >= L is causal, and causal refuses a padding and a padding mode"
    else:
        if has(longn="64x64", row=("mid", "big")) or has(longn=("64x128", "128x64"), row="big"):
            return "ValueError of the library: the forced N1 x N2 holds fewer points than the row needs"
    return None


def test_every_pair_left_out_is_refused_for_a_stated_reason():
    """``allowed_pairs`` finds what is allowed by trial; what it leaves out must be refused by a rule, not merely rare."""
    for kind in ("fwd", "tr"):
        axes = {a: v for a, v in su.AXES[kind].items() if a not in su.STEERING}
        names = list(axes)
        allowed = su.allowed_pairs(kind)
        left_out = [(a, va, b, vb) for i, a in enumerate(names) for b in names[i + 1:] for va in axes[a] for vb in axes[b]
                    if (a, va, b, vb) not in allowed]
        unexplained = [q for q in left_out if _why_refused(kind, *q) is None]
        assert not unexplained, f"{kind}: left out without a rule: {unexplained}"
        wrongly = [q for q in allowed if _why_refused(kind, *q) is not None]
        assert not wrongly, f"{kind}: allowed against a rule: {wrongly[:8]}"
        assert len(left_out) == {"fwd": 23, "tr": 9}[kind], (kind, len(left_out))


def test_pairs_the_rule_refuses_are_refused_by_the_api():
    """What ``allowed_pairs`` leaves out is what the contract refuses: spot checks against the calls' own argument errors."""
    fwd = su.allowed_pairs("fwd")
    for q in (("padding", "same", "stride", 2), ("causal", True, "mode", "reflect"), ("causal", True, "padding", "odd"),
              ("kclass", "row", "causal", False), ("groups", "dw", "cig", 2), ("grads", False, "dy", "nlc")):
        a, va, b, vb = q
        assert q not in fwd and (b, vb, a, va) not in fwd, q
    x, w = torch.zeros(1, 1, 6000), torch.zeros(1, 1, 100)
    with pytest.raises(ValueError, match="strided"):
        F_.fft_long_conv(x, w, padding="same", stride=2)
    with pytest.raises(ValueError, match="padding_mode must be 'constant'"):
        F_.fft_long_conv(x, w, causal=True, padding_mode="reflect")
    with pytest.raises(ValueError, match="padding must be 0"):
        F_.fft_long_conv(x, w, causal=True, padding=3)
    assert ("stride", 1, "opad", "1") in su.allowed_pairs("tr")          # (through the dilation)
    with pytest.raises(ValueError, match="output_padding"):
        F_.fft_long_conv_transpose(x, w, None, 1, 0, 1, 1)


QUOTAS = {"fwd handoff": 3, "fwd plain": 12, "fwd phases": 8, "dW plan": 6, "dW exchanged": 6, "dW by phases": 3,
          "tr handoff": 2, "tr phases": 6, "tr spread": 6, "tr dX by decimation": 3, "tr dW by decimation": 3, "slabs >= 2": 8,
          "klo > 0": 3, "y = bias only": 1, "tr dropped leading samples": 2, **{"N " + n: 2 for n in su.FORCED_N}}


def test_routes_the_library_predicts_meet_their_quotas_and_the_records_agree(monkeypatch):
    have = collections.Counter()
    for c in _all():
        _switch(monkeypatch, c)
        pred = su.predict(c)
        assert pred["route"] == c.route, c.id
        have[f"{c.kind} {pred['route']}"] += 1
        ran = pred["route"] != "handoff"
        if c.kind == "fwd" and c.grads and ran:
            have["dW by phases" if pred["dw_phases"] else f"dW {pred['dw']}"] += 1
        have["tr dX by decimation"] += pred["dx_decim"]
        have["tr dW by decimation"] += pred["dw_decim"]
        have["slabs >= 2"] += c.slabs >= 2
        if c.forced and ran:
            have["N " + dict(c.env)[su.KNOBS["longn"]]] += 1
        if c.kind == "fwd":
            have["klo > 0"] += 0 < c.klo <= c.khi
            have["y = bias only"] += c.khi < c.klo
        have["tr dropped leading samples"] += c.kind == "tr" and c.drop > 0 and pred["route"] == "spread"
        # the record's plan is the library's under these switches
        mode = _native.PAD_MODES[c.mode]
        info = None
        if c.kind == "fwd" and c.route == "plain":
            key = (c.B, c.cin, c.cout, c.groups, c.L, c.K, c.pl, c.pr, F_._long_keep(c.L, c.causal, c.stride), int(c.causal),
                   int(c.bias), mode, 1, c.dilation, c.stride) + ((_native.LONG_COMPLEX,) if c.complex else ())
            info = _native.long_geometry(key)
            assert info["out_len"] == c.nout, c.id
        elif c.kind == "fwd" and c.route == "phases":
            info = _native.decim_geometry((c.B, c.cin, c.cout, c.groups, c.L, c.K, c.stride, c.pl, c.pr,
                                           F_._long_keep(c.L, c.causal, c.stride), int(c.causal), int(c.bias)))
        elif c.route == "phases":
            info = _native.phases_geometry((c.B, c.cin, c.cout, c.groups, c.L, c.K, c.stride, c.padding, c.opad, int(c.bias)))
            assert info["out_len"] == c.nout, c.id
        elif c.route == "spread":
            drop, n, lead, tail = F_._long_spread_args(c.L, c.K, c.stride, c.padding, c.opad, c.dilation)
            assert drop == c.drop
            key = (c.B, c.cin, c.cout, c.groups, n, c.K, lead, tail, c.nout, 1, int(c.bias), 0, c.stride, c.dilation, 1) + \
                ((_native.LONG_COMPLEX,) if c.complex else ())
            info = _native.long_geometry(key)
        if info is None:
            assert c.n1n2 is None and c.slabs == 0, c.id
        else:
            assert (info["N1"], info["N2"]) == c.n1n2 and info["slabs"] == c.slabs and info["slab_pairs"] == c.slab_pairs, \
                (c.id, info, c.n1n2, c.slabs)
            if c.forced:
                assert c.n1n2 == c.forced, c.id
            if c.slabs >= 2:
                assert dict(c.env).get(su.KNOBS["ws"]) == "1" and (c.B >= 3 or c.complex), c.id
    print({k: have[k] for k in QUOTAS})
    short = {k: (have[k], n) for k, n in QUOTAS.items() if have[k] < n}
    assert not short, f"quotas not met (have, need): {short}"


# ------------------------------------------------------------------------------------------------ exactness, fault models
def _partial(c, x, w, b, gy, items):
    """dW of the batch items ``items`` alone (exact)."""
    return su.truth(c, x[items], w, b, gy[items])["dW"]


def _out_block(c):
    """out_block of the plain plan of the case's forward shape."""
    if c.kind == "fwd":
        key = (c.B, c.cin, c.cout, c.groups, c.L, c.K, c.pl, c.pr, F_._long_keep(c.L, c.causal, c.stride), int(c.causal),
               int(c.bias), _native.PAD_MODES[c.mode], 1, c.dilation, c.stride)
    else:
        drop, n, lead, tail = F_._long_spread_args(c.L, c.K, c.stride, c.padding, c.opad, c.dilation)
        key = (c.B, c.cin, c.cout, c.groups, n, c.K, lead, tail, c.nout, 1, int(c.bias), 0, c.stride, c.dilation, 1)
    return _native.long_geometry(key)["out_block"]


def _defects(c, x, w, b, gy, want):
    """(name, the truth with one defect) for every fault model that changes a value of this case."""
    y = want["y"]
    out = []

    def put(name, **changed):
        new = dict(want, **changed)
        if any(not torch.equal(new[k], want[k]) for k in changed):
            out.append((name, new))
    w2 = w.clone()
    w2[..., -1] = 0
    put("the last tap dropped", y=su.truth(c, x, w2, b, None)["y"])
    put("the result shifted by one sample", y=torch.roll(y, 1, -1))
    if c.B % 2 and c.B >= 3:
        t = y.clone()
        t[-1] = t[-2]
        put("the odd batch item replaced by its pair partner", y=t)
    if c.cog >= 2:
        t = y.clone()
        t[:, [0, 1]] = y[:, [1, 0]]
        put("two channels of one group swapped", y=t)
    if c.complex:
        put("the imaginary part negated", y=y.conj().resolve_conj())
    ob = _out_block(c)
    if c.cout % ob:
        t = y.clone()
        t[:, c.cout // ob * ob] = 0
        put("the first out_block remainder channel zeroed", y=t)
    if c.grads:
        if c.slabs >= 2:
            first = 2 * c.slab_pairs * (c.slabs - 1) if not c.complex else c.slab_pairs * (c.slabs - 1)
            put("one slab's contribution to dW missing", dW=want["dW"] - _partial(c, x, w, b, gy, slice(first, c.B)))
        t = want["dX"].clone()
        t[..., :max(1, min(c.L, c.pl))] += 1
        put("dX of the leading pad_left region nonzero", dX=t)
    return out


CAUGHT = collections.defaultdict(list)          # fault model -> ids of the cases that caught it (printed at the end)
DONE = set()
CHUNKS = [(kind, n) for kind, table in zip(("fwd", "tr"), su.tables()) for n in range(0, len(table), CHUNK)]


@pytest.mark.parametrize("kind,first", CHUNKS, ids=[f"{k}{n:02d}" for k, n in CHUNKS])
def test_truth_is_exact_and_the_checker_rejects_every_fault_model(kind, first):
    cases = su.tables()[0 if kind == "fwd" else 1][first:first + CHUNK]
    assert cases
    for c in cases:
        x, w, b, gy = su.inputs(c)
        # the bound of accuracy_util.assert_exact, restated for the long arguments
        xmax = (au.HI if c.tdtype != torch.float16 else au.HI // su.F16_DIV) + \
               (0 if c.cls != "offset" else au.OFFSET if c.tdtype != torch.float16 else su.F16_OFFSET)
        per_group, rows = max(c.cig, c.cog), c.B * max(c.nout, c.L)
        bound = max(xmax * au.HI * c.K * per_group + au.HI, xmax * au.HI * rows) * (2 if c.complex else 1)
        assert bound < au.EXACT_LIMIT, c.id
        for t in (x, w, b, gy):
            if t is not None:
                r = torch.view_as_real(t) if t.is_complex() else t
                assert t.dtype == c.tdtype and au.is_whole(r.double()) and r.abs().max() <= xmax, c.id
        want = su.truth(c, x, w, b, gy)
        assert tuple(want["y"].shape) == (c.B, c.cout, c.nout), c.id
        assert all(v is None or au.is_whole(v) for v in want.values()), c.id
        js = su.sample_positions(c)
        assert {0, c.nout - 1} <= set(js)
        at = want["y"][[0, c.B - 1]][:, :, js]
        assert torch.equal(at, su.dots(c, x, w, b, js)), f"{c.id}: the truth differs from explicit dot products"
        if c.khi < c.klo:
            assert torch.equal(want["y"], torch.zeros_like(want["y"]) + (0 if b is None else su.wide(b)[None, :, None])), c.id
        if c.tdtype == torch.float16:
            top = max(float(v.abs().max()) for v in want.values() if v is not None)
            assert top < su.F16_MAX, f"{c.id}: the exact result reaches {top}"
        if c.kind == "tr" and c.B * c.cin * c.cog * c.L * c.K <= 2e8 and not c.complex:
            ref = F.conv_transpose1d(su.wide(x), su.wide(w), su.wide(b), c.stride, c.padding, c.opad, c.groups, c.dilation)
            assert torch.equal(want["y"], ref), c.id
        # the checker: accepts the baseline, rejects every defect
        base = su.baseline(c, x, w, b, gy)
        su.check_values(c, base, want, base, " (the baseline itself)")
        for name, broken in _defects(c, x, w, b, gy, want):
            with pytest.raises(AssertionError):
                su.check_values(c, broken, want, base, f" ({name})")
            CAUGHT[name].append(c.id)
    DONE.add((kind, first))
    if len(DONE) == len(CHUNKS):          # (a run of the whole file: every fault model was rejected somewhere)
        for name, ids in CAUGHT.items():
            print(f"fault model '{name}': rejected on {len(ids)} cases, e.g. {ids[0]}")
        assert len(CAUGHT) == 8, sorted(CAUGHT)


# ------------------------------------------------------------------------------------------------ determinism
def _digest(tables):
    return hashlib.sha256(repr([dataclasses.astuple(c) for t in tables for c in t]).encode()).hexdigest()


def test_table_is_the_same_in_another_process_with_another_hash_seed():
    here = _digest(su.tables())
    again = _digest(su.tables.__wrapped__(su.SEED))      # a second construction, not the cached one
    assert here == again
    env = dict(os.environ, PYTHONHASHSEED="12345" if os.environ.get("PYTHONHASHSEED") != "12345" else "54321")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_host_long_sweep as t, long_sweep_util as su\n"
            "print(t._digest(su.tables()))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, cwd=ROOT)
    assert out.stdout.strip().splitlines()[-1] == here


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular", "constant"])
def test_sliced_padding_of_the_baseline_is_torchs_padding(mode):
    x = torch.arange(2 * 3 * 11, dtype=torch.float64).reshape(2, 3, 11)
    for pl, pr in ((0, 0), (3, 3), (4, 5), (10, 0), (0, 10)) + (((11, 11),) if mode != "reflect" else ()):
        assert torch.equal(su.pad(x, pl, pr, mode), F.pad(x, (pl, pr), mode=mode) if pl or pr else x), (mode, pl, pr)
    xr = x.clone().requires_grad_()
    su.pad(xr, 10, 10, mode).sum().backward()
    ref = x.clone().requires_grad_()
    F.pad(ref, (10, 10), mode=mode).sum().backward()
    assert torch.equal(xr.grad, ref.grad)
