"""Route table of tests/test_gpu_routes.py: which kernel build each case must run (``Plan.route``, fc_debug_route), the
knobs it needs, and the helpers that check a case against float64 -- the seam probe, element-wise errors and sampled
float64 dot products for outputs too large for a full reference.

A route is (name, knobs, predicate on ``Plan.route``, cases).  Knobs are environment variables read at plan creation;
a case may add its own (``env``; None unsets one).  ``expect`` is a further predicate of one case (a tile count the
case was sized for)."""
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

TOL32 = 1e-4        # float32 plans: max|got - want| / max|want|, the project's bound
TOL64 = 1e-12       # float64 plans
FULL_REF_MAX = 1 << 24    # outputs up to this many samples get a full float64 reference, larger ones sampled dot products


@dataclass
class Case:
    B: int
    cin: int
    cout: int
    size: tuple
    k: tuple
    s: object = 1
    p: object = 0
    d: object = 1
    g: int = 1
    mode: str = "constant"
    tr: bool = False              # fft_conv_transpose (weight (Cin, Cout/g, *k))
    op: object = 0                # output_padding (transposed)
    f64: bool = False
    grads: bool = False           # dX / dW / db through autograd against float64 autograd
    public: bool = False          # also through fft_conv / fft_conv_transpose
    env: dict = field(default_factory=dict)
    expect: Optional[Callable] = None
    note: str = ""

    @property
    def nd(self):
        return len(self.size)

    def tup(self, v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * self.nd

    @property
    def wshape(self):
        if self.tr:
            return (self.cin, self.cout // self.g) + tuple(self.k)
        return (self.cout, self.cin // self.g) + tuple(self.k)

    def ident(self):
        t = "T" if self.tr else ""
        return (f"{t}B{self.B}c{self.cin}-{self.cout}g{self.g}s{'x'.join(map(str, self.size))}"
                f"k{'x'.join(map(str, self.k))}{self.mode[:4]}" + (f"-{self.note}" if self.note else ""))


@dataclass
class Route:
    name: str
    env: dict
    pred: Callable
    cases: list


def _words(kind, want):
    """Predicate: the plan is of this kind and these route words have exactly these values.  Counts such as nxt are 1
    on an untiled axis, so a truth value says nothing: a tile count is compared in a lambda (r["nxt"] > 1)."""
    for k, v in want.items():
        if not isinstance(v, int) or isinstance(v, bool):
            raise TypeError(f"route word {k} must be compared with an int, got {v!r}")

    def pred(r):
        return r["kind"] == kind and all(r[k] == v for k, v in want.items())
    return pred


def _1d(**want):
    return _words("f32_1d", want)


def _nd(**want):
    return _words("f32_nd", want)


def _f64(kind, **want):
    return _words(kind, want)


def fusedc_nb(r, B, cog, G=1):
    """Batch items per workgroup of the 2-D fused column pass as launch_fusedc's batch and grid conditions decide them:
    the largest of 4 and 2 that is at most B and still leaves a grid of 512 workgroups, else 1.  (The launch also needs
    the tile's build to fit NB x CIB sequences in its threads and LDS; that is a property of the compiled tile.)"""
    ncol = r["Tx"] // 2 * r["nxt"]
    chunks = -(-cog // r["cob"])
    for nb in (4, 2):
        if nb <= B and -(-B // nb) * r["ntiles"] * chunks * G * ncol >= 512:
            return nb
    return 1


def tail_split(r, B, nb, G=1):
    """build_work_list's tail split: full items (nb batch items that share a tile and an out-chunk) in excess of whole
    residency rounds are halved when they fill at most half a round.  True if pers_items is what that rule gives for one
    of the possible slot counts (CUs x resident workgroups per CU) and a split happened."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    units = r["n_ochunks"] * G
    full = (B // nb) * r["ntiles"] * units
    unsplit = full + (r["ntiles"] * units if B % nb else 0)
    extra = r["pers_items"] - unsplit
    if extra <= 0:
        return False
    for wgs in range(1, 9):
        slots = cus * wgs
        if full > slots and full % slots == extra and extra <= slots // 2:
            return True
    return False


C = Case
TAIL_SPLIT_CASES = [
    # 300 tiles of 896 valid samples (1024-point tiles, k 129): 600 full items of two batch items, more than one round
    C(4, 8, 8, (300 * 896 + 128,), (129,), grads=True, public=True, expect=lambda r: tail_split(r, 4, 2)),
    C(5, 8, 8, (300 * 896 + 128 - 40,), (129,), p=20, mode="reflect", note="rem1", expect=lambda r: tail_split(r, 5, 2)),
]

ROUTES = [
    # ------------------------------------------------------------------------------------------------ float32 1-D
    Route("1d-general-single", {}, _1d(pers_nb=0, accumulate=0, chunk_launches=0, wide=0, dense=0, nseg=1), [
        C(3, 4, 6, (3001,), (65,), p=32, grads=True, public=True),
        C(2, 8, 8, (4000,), (33,), s=2, p=16, mode="reflect", note="stride2"),
        C(5, 8, 12, (2500,), (17,), p=8, mode="replicate"),
        C(4, 6, 10, (1800,), (40,), s=3, p=20, mode="circular"),
        C(2, 8, 6, (700,), (33,), s=2, p=5, op=1, tr=True, public=True, grads=True),
        C(2, 8, 6, (961,), (65,), env={"FFTCONV_TILE": "512"}, note="last-tile-1",
          expect=lambda r: r["T"] == 512 and r["ntiles"] == 3),
        C(3, 8, 6, (1408,), (65,), env={"FFTCONV_TILE": "512"}, mode="reflect", p=0, note="exact-V",
          expect=lambda r: r["T"] == 512 and r["ntiles"] == 3),
    ]),
    Route("1d-general-running-sum", {}, _1d(pers_nb=0, accumulate=1, chunk_launches=0, wide=0, dense=0, nseg=1), [
        C(2, 9, 6, (3001,), (33,), p=16, grads=True, public=True),
        C(3, 17, 5, (2000,), (50,), p=10, mode="reflect"),
        C(2, 16, 16, (1500,), (33,)),
        C(2, 12, 8, (3000,), (31,), s=2, p=15, mode="circular"),
        C(2, 9, 7, (1000,), (20,), p=3, mode="replicate"),
    ]),
    Route("1d-chunk-launches", {}, _1d(chunk_launches=1, pers_nb=0), [
        C(2, 20, 6, (5317,), (700,), p=100, d=3, grads=True, public=True),
        C(1, 9, 4, (4000,), (1100,), d=2),
        C(2, 17, 6, (6000,), (2100,), p=50, mode="reflect"),
        C(1, 16, 5, (5000,), (2500,), p=7, mode="circular"),
    ]),
    Route("1d-pers-1024-nb2", {"FFTCONV_PERS": "2"}, _1d(T=1024, pers_nb=2, slot_tiles=0, ph=1, wide=0, nseg=1), [
        C(3, 8, 8, (1921,), (129,), grads=True, public=True, note="last-tile-1", expect=lambda r: r["ntiles"] == 3),
        C(8, 8, 8, (2816,), (129,), mode="reflect", note="exact-V"),
        C(2, 16, 16, (5000,), (129,), g=2, p=64, mode="circular"),
        C(5, 8, 8, (3000,), (200,), p=99, mode="replicate"),
    ]),
    Route("1d-pers-1024-nb4", {"FFTCONV_PERS": "4"}, _1d(T=1024, pers_nb=4, slot_tiles=0, ph=1, wide=0, nseg=1), [
        C(5, 8, 8, (1921,), (129,), grads=True, public=True, note="rem1"),
        C(6, 8, 8, (2816,), (129,), mode="reflect", note="rem2"),
        C(7, 8, 8, (4000,), (65,), p=32, mode="circular", note="rem3"),
        C(4, 16, 16, (3000,), (257,), g=2, p=1, mode="replicate"),
    ]),
    Route("1d-pers-2048-nb1", {"FFTCONV_PERS": "1"}, _1d(T=2048, pers_nb=1, wide=0, nseg=1), [
        C(3, 8, 8, (2 * 1449 + 600,), (600,), grads=True, public=True, note="last-tile-1"),
        C(2, 8, 8, (6000,), (900,), p=100, mode="reflect"),
        C(1, 8, 16, (5000,), (1000,), p=5, mode="circular"),
    ]),
    Route("1d-pers-2048-nb2", {"FFTCONV_PERS": "2"}, _1d(T=2048, pers_nb=2, slot_tiles=0, wide=0, nseg=1), [
        C(3, 8, 8, (3 * 1149 + 899,), (900,), grads=True, public=True, note="exact-V"),
        C(5, 8, 8, (7000,), (1000,), p=300, mode="replicate"),
        C(4, 8, 8, (5000,), (800,), p=10, mode="circular"),
    ]),
    Route("1d-slot-tiles", {"FFTCONV_PERS": "4"}, _1d(T=1024, pers_nb=4, slot_tiles=1), [
        C(1, 8, 8, (9 * 768 + 256,), (257,), grads=True, public=True, note="9-tiles", expect=lambda r: r["ntiles"] == 9),
        C(3, 8, 8, (6 * 768 + 1 + 256,), (257,), note="last-tile-1", expect=lambda r: r["ntiles"] == 7),
        C(2, 8, 8, (3000,), (257,), p=100, mode="reflect"),
        C(1, 16, 16, (20000,), (129,), g=2, p=64, mode="circular"),
        C(2, 8, 8, (7000,), (300,), p=5, mode="replicate"),
    ]),
    Route("1d-tail-split", {"FFTCONV_PERS": "2"}, _1d(T=1024, pers_nb=2, slot_tiles=0), TAIL_SPLIT_CASES),
    Route("1d-phases-single", {"FFTCONV_PERS": "4", "FFTCONV_PH2": "0"}, lambda r: _1d(ph2=0)(r) and r["ph"] > 1, []),
    Route("1d-phases-pairs", {"FFTCONV_PERS": "4", "FFTCONV_PH2": "1"}, lambda r: _1d(ph2=1)(r) and r["ph"] > 1, []),
    Route("1d-phases-quads", {"FFTCONV_PERS": "4"}, lambda r: _1d(ph2=2)(r) and r["ph"] % 4 == 0, []),
    Route("1d-depthwise", {}, _1d(diag=1, ph=1, nseg=1), [
        C(3, 24, 24, (5000,), (33,), g=24, p=5, mode="reflect", grads=True, public=True),
        C(4, 12, 12, (2000,), (65,), g=12),
        C(3, 5, 5, (3000,), (129,), g=5, p=7, mode="replicate"),
        C(1, 8, 8, (100000,), (257,), g=8, mode="circular", p=100),
    ]),
    Route("1d-depthwise-phases", {"FFTCONV_PERS": "4"}, lambda r: _1d(diag=1, nseg=1)(r) and r["ph"] > 1, [
        C(5, 16, 16, (9000,), (200,), g=16, p=64, d=4, mode="circular", grads=True, public=True),
        C(2, 21, 21, (2500,), (300,), g=21, d=3),
        C(3, 8, 8, (8001,), (65,), g=8, d=13, p=10, mode="reflect"),
    ]),
    Route("1d-segments", {}, lambda r: _1d(diag=0)(r) and r["nseg"] > 1, [
        C(2, 8, 8, (20000,), (5000,), grads=True, public=True),
        C(2, 12, 8, (15000,), (4500,), p=100, mode="circular"),
        C(1, 8, 8, (8192,), (8192,), p=4096),
        C(3, 4, 6, (12000,), (3000,), p=50, d=2, mode="reflect"),
    ]),
    Route("1d-segments-depthwise", {}, lambda r: _1d(diag=1)(r) and r["nseg"] > 1, [
        C(2, 16, 16, (9000,), (2048,), g=16, grads=True, public=True),
        C(1, 8, 8, (7000,), (3000,), g=8, p=20, mode="replicate"),
    ]),
    Route("1d-block-diagonal-gs2", {}, _1d(bd_gs=2), [
        C(4, 16, 16, (20000,), (257,), g=8, grads=True, public=True),
        C(2, 24, 24, (3000,), (65,), g=12, p=10, mode="circular", env={"FFTCONV_PERS": "2"}),
        C(3, 8, 8, (5000,), (129,), g=4, p=3, mode="replicate", env={"FFTCONV_PERS": "2"}),
    ]),
    Route("1d-block-diagonal-gs4", {}, _1d(bd_gs=4), [
        C(3, 32, 32, (9000,), (129,), g=8, p=30, mode="reflect", grads=True, public=True, env={"FFTCONV_PERS": "2"}),
        C(5, 8, 8, (5000,), (513,), g=2, d=2),
    ]),
    Route("1d-wide-1024", {}, _1d(wide=1, T=1024), [
        C(3, 16, 8, (5000,), (100,), p=16, mode="reflect", grads=True, public=True),
        C(7, 9, 8, (1200,), (97,), p=2, note="rem1"),
        C(2, 17, 16, (3000,), (300,), p=20, mode="circular"),
    ]),
    Route("1d-wide-2048", {}, _1d(wide=1, T=2048), [
        C(4, 32, 32, (9000,), (1025,), g=2, p=100, mode="replicate", grads=True, public=True),
        C(3, 17, 8, (4000,), (800,)),
    ]),
    Route("1d-dense-1024", {}, _1d(dense=1, T=1024), [
        C(4, 64, 64, (9000,), (129,), p=64, grads=True, public=True),
        C(3, 17, 16, (3000,), (65,), env={"FFTCONV_DENSE": "2"}, p=10, mode="reflect"),
        C(2, 16, 24, (5000,), (100,), g=1, env={"FFTCONV_DENSE": "2"}, mode="circular", p=7),
        C(6, 32, 32, (4000,), (33,), env={"FFTCONV_DENSE": "2", "FFTCONV_DENSE_SLAB": "5"}, mode="replicate", p=16, note="slabs"),
    ]),
    Route("1d-dense-2048", {}, _1d(dense=1, T=2048), [
        C(2, 32, 48, (6000,), (1000,), env={"FFTCONV_DENSE": "2"}, grads=True, public=True),
        C(3, 16, 16, (5000,), (800,), env={"FFTCONV_DENSE": "2", "FFTCONV_DENSE_SLAB": "2"}, p=40, mode="reflect",
          note="slabs"),
    ]),
    # ------------------------------------------------------------------------------------------------ float32 N-d
    Route("2d-separable-cob2", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=2, Tm=0), [
        C(5, 2, 2, (60, 400), (5, 5), p=2, grads=True, public=True, note="nb4", expect=lambda r: fusedc_nb(r, 5, 2) == 4),
        C(3, 1, 2, (60, 400), (5, 3), p=(2, 1), mode="reflect", note="nb2", expect=lambda r: fusedc_nb(r, 3, 2) == 2),
        C(1, 2, 2, (50, 70), (3, 5), s=2, p=1, mode="circular", note="nb1"),
    ]),
    Route("2d-separable-cob4", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=4, Tm=0), [
        C(5, 3, 4, (60, 400), (5, 5), p=2, mode="replicate", grads=True, public=True, note="nb4",
          expect=lambda r: fusedc_nb(r, 5, 4) == 4),
        C(3, 4, 4, (40, 500), (3, 3), p=1, note="nb2", expect=lambda r: fusedc_nb(r, 3, 4) == 2),
        C(1, 3, 4, (33, 45), (4, 2), s=(2, 3), p=(1, 0)),
    ]),
    Route("2d-separable-cob8", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=8, Tm=0), [
        C(5, 8, 8, (40, 400), (5, 5), p=2, grads=True, public=True, note="nb4", expect=lambda r: fusedc_nb(r, 5, 8) == 4),
        C(3, 6, 9, (40, 500), (3, 7), p=(1, 3), mode="reflect", note="cog9-nb2", expect=lambda r: fusedc_nb(r, 3, 9) == 2),
        C(1, 16, 12, (30, 60), (3, 3), s=2, p=1, mode="circular", note="nb1"),
        C(2, 17, 8, (20, 50), (3, 3), p=1, mode="replicate", note="cig17"),
    ]),
    Route("2d-x-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0, Tm=0)(r) and r["nxt"] > 1, [
        C(2, 4, 4, (30, 512), (3, 7), p=(1, 3), grads=True, public=True),
        C(1, 2, 3, (8, 5000), (3, 65), p=(1, 32)),
        C(2, 3, 2, (20, 700), (3, 5), p=(1, 2), mode="reflect", s=(1, 2)),
    ]),
    Route("2d-outer-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0, Tm=0)(r) and r["ntiles"] > 1, [
        C(1, 2, 3, (3000, 9), (40, 3), p=(5, 1), s=(3, 1), mode="reflect", grads=True, public=True),
        C(2, 4, 4, (2000, 20), (65, 3), p=(32, 1), mode="circular"),
    ]),
    Route("2d-colz-b1", {"FFTCONV_PLANES": "2"}, _nd(planes=2), [
        C(1, 8, 8, (100, 200), (5, 5), p=2, grads=True, public=True),
        C(1, 6, 5, (64, 130), (3, 3), p=1, mode="reflect"),
        C(1, 8, 16, (70, 100), (5, 3), s=2, p=(2, 1), mode="circular"),
    ]),
    Route("2d-colz-b2", {"FFTCONV_PLANES": "2"}, _nd(planes=2), [
        C(2, 8, 8, (100, 200), (5, 5), p=2, grads=True, public=True),
        C(3, 6, 5, (64, 130), (3, 3), p=1, mode="replicate"),
        C(5, 16, 8, (40, 96), (7, 3), g=2, p=(3, 1)),
    ]),
    Route("3d-separable-y-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0)(r) and r["nyt"] > 1, [
        C(1, 2, 3, (8, 518, 20), (3, 7, 3), p=(1, 3, 1), grads=True, public=True),
        C(2, 4, 4, (6, 600, 10), (3, 5, 3), p=(1, 2, 1), mode="reflect"),
    ]),
    Route("3d-planes-untiled", {}, lambda r: _nd(planes=1)(r) and r["nxt"] * r["nyt"] == 1, [
        C(2, 8, 8, (20, 40, 40), (3, 3, 3), p=1, grads=True, public=True),
        C(1, 8, 16, (30, 33, 47), (5, 3, 2), s=(2, 1, 3), p=(2, 1, 0)),
        C(3, 6, 6, (17, 33, 20), (2, 3, 3), s=(1, 2, 1), p=1, mode="replicate"),
    ]),
    Route("3d-planes-tiled", {}, lambda r: _nd(planes=1, Tx=64, Tm=64)(r) and r["nxt"] * r["nyt"] > 1, [
        C(2, 8, 8, (40, 100, 130), (3, 5, 5), p=2, grads=True, public=True),
        C(1, 8, 8, (20, 340, 340), (3, 3, 3), p=1, note="36-tiles", expect=lambda r: r["nxt"] * r["nyt"] == 36),
        C(2, 8, 16, (30, 70, 90), (5, 3, 7), s=(1, 2, 3), p=(2, 1, 3), mode="reflect"),
    ]),
    # the 64 x 64 tiles of the plane-major pipeline are chosen before its offset guard is known: past the guard the
    # separable passes run them, with more middle-axis tiles than their own planner allows (8)
    Route("3d-64-tiles-past-the-guard", {}, lambda r: _nd(planes=0, Tx=64, Tm=64)(r) and r["nyt"] > 8, [
        C(1, 8, 32, (56, 500, 64), (3, 3, 3), p=1, grads=True, public=True, expect=lambda r: r["nxt"] * r["nyt"] == 18),
    ]),
    Route("3d-planes-below-the-guard", {}, lambda r: _nd(planes=1, Tx=64, Tm=64)(r) and r["nyt"] > 8, [
        C(1, 8, 32, (54, 500, 64), (3, 3, 3), p=1, expect=lambda r: r["nxt"] * r["nyt"] == 18),
    ]),
    # ------------------------------------------------------------------------------------------------ float64
    Route("f64-direct", {}, _f64("f64_direct"), [
        C(2, 3, 4, (20, 30), (3, 3), p=1, mode="reflect", f64=True, grads=True, public=True),
        C(3, 4, 6, (500,), (9,), s=2, p=4, mode="circular", f64=True),
        C(2, 2, 2, (6, 7, 8), (2, 3, 2), p=1, f64=True),
    ]),
    Route("f64-1d-fft", {}, _f64("f64_fft_1d"), [
        C(3, 4, 6, (3001,), (65,), p=32, mode="reflect", f64=True, grads=True, public=True),
        C(2, 6, 4, (700,), (33,), s=2, p=5, op=1, tr=True, f64=True, grads=True, public=True),
        C(2, 8, 3, (4000,), (20,), s=3, p=9, mode="replicate", f64=True),
        C(1, 2, 2, (1000,), (100,), g=2, p=50, mode="circular", f64=True),
    ]),
    Route("f64-nd-nb1", {}, _f64("f64_fft_nd", nb=1), [
        C(2, 4, 9, (30, 40), (7, 7), p=3, f64=True, grads=True, public=True, note="cog9"),
        C(1, 4, 2, (30, 40), (7, 7), p=3, mode="circular", f64=True),
        C(2, 4, 6, (10, 12, 9), (3, 3, 3), p=1, mode="reflect", f64=True),
    ]),
    Route("f64-nd-nb2", {}, _f64("f64_fft_nd", nb=2), [
        C(3, 4, 3, (30, 40), (7, 7), p=3, f64=True, grads=True, public=True),
        C(2, 9, 4, (21, 33), (7, 7), s=2, p=3, mode="replicate", f64=True),
        C(2, 6, 4, (9, 10, 11), (3, 3, 4), g=2, p=1, mode="circular", f64=True),
    ]),
    Route("f64-nd-nb4", {}, _f64("f64_fft_nd", nb=4), [
        C(5, 4, 2, (30, 40), (7, 7), p=3, f64=True, grads=True, public=True, note="rem1"),
        C(3, 4, 2, (30, 40), (7, 7), p=3, mode="circular", f64=True, note="B<nb"),
        C(6, 4, 2, (25, 31), (7, 7), mode="reflect", p=2, f64=True, note="rem2"),
        C(7, 6, 2, (8, 10, 12), (3, 3, 3), p=1, mode="replicate", f64=True, note="rem3"),
        C(4, 4, 4, (20, 22), (7, 8), g=2, p=1, f64=True, note="g2"),
    ]),
    Route("f64-nd-spectrum-32mib", {}, _f64("f64_fft_nd", nb=2, cob=4), [
        C(3, 12, 6, (248, 248), (9, 9), p=4, f64=True, grads=True, public=True),
        C(2, 13, 5, (248, 248), (9, 9), p=4, mode="reflect", f64=True),
    ]),
    Route("f64-2048-tiles", {}, lambda r: (r["kind"] == "f64_fft_1d" and r["T"] == 2048) or
          (r["kind"] == "f64_fft_nd" and 2048 in (r["t0"], r["t1"], r["t2"])), [
        C(2, 2, 3, (5000,), (600,), p=10, f64=True, grads=True, public=True),
        C(1, 1, 2, (10, 2500), (3, 513), p=(1, 0), d=(1, 2), f64=True),
    ]),
]

# dilation phases: the same shapes under FFTCONV_PH2 0 / 1 / default (singles, pairs, quads)
# (dilated extents past 769: the 1024-point batch-sharing tile cannot take the dilated kernel, so FFTCONV_PERS=4 leaves
#  the phases as its only candidate; at shorter extents the two tie within one residency round and the planner keeps the
#  dilated kernel)
PHASE_CASES = [
    C(8, 8, 8, (40001,), (200,), d=4, note="L%4=1"),
    C(4, 8, 8, (30002,), (250,), d=4, p=31, mode="reflect"),
    C(2, 8, 8, (50000,), (129,), d=8, p=64, mode="circular"),
    C(5, 8, 8, (9001,), (200,), d=4, p=4, mode="replicate"),
    C(3, 16, 16, (20003,), (100,), g=2, d=12, p=7),
]
for _r in ROUTES:
    if _r.name.startswith("1d-phases"):
        _r.cases.extend(PHASE_CASES)
        _r.cases[0] = Case(**{**_r.cases[0].__dict__, "grads": True, "public": True})


# ---------------------------------------------------------------------------------------------------------------------
# dX of a strided convolution is a transposed plan with up > 1: the input spread over the stride's grid.  Strided transposed
# plans on every route that takes them (tests/test_gpu_backward_routes.py runs them through test_gpu_routes._run_case).
# A list of its own: the files that walk ROUTES do not see these cases.
def tile_step(c, r, ax):
    """(valid outputs per tile, tiles) of axis ax of a plan, from its route words (a segmented 1-D plan: the tile holds
    one segment's extent)."""
    kd = (c.k[ax] - 1) * c.tup(c.d)[ax] + 1
    kind = r["kind"]
    if kind in ("f32_1d", "f64_fft_1d"):
        T, n = r["T"], r["ntiles"]
        if r.get("nseg", 1) > 1:
            # segments of taps (decide_route): 1024 // d + 1 taps each, an extent of at most 1025 samples per segment
            d = c.tup(c.d)[ax]
            seg_taps = min(max(1, 1024 // d + 1), c.k[ax])
            assert -(-c.k[ax] // seg_taps) == r["nseg"], (seg_taps, r)
            kd = (seg_taps - 1) * d + 1
    elif kind == "f32_nd":
        T, n = ((r["T"], r["ntiles"]) if ax == 0 else (r["Tx"], r["nxt"]) if ax == c.nd - 1 else (r["Tm"], r["nyt"]))
    else:
        T, n = r[f"t{ax}"], r[f"nt{ax}"]
    return T - kd + 1, n


def seam_phases(c, r, ax):
    """Where the tile seams of axis ax of a strided transposed plan sit on the stride's grid: input sample i lies at
    kd - 1 - p + i * s of the padded row whose window [o, o + kd) gives output o, tile j starts at output j * V.  The set of
    (j * V - (kd - 1 - p)) mod s over the seams; {0}: every seam on the grid."""
    kd = (c.k[ax] - 1) * c.tup(c.d)[ax] + 1
    V, n = tile_step(c, r, ax)
    return {(j * V - (kd - 1 - c.tup(c.p)[ax])) % c.tup(c.s)[ax] for j in range(1, n)}


def _t(*a, grid=None, **kw):
    """A transposed case; grid=(axis, on), or a list of them: the case is sized so that the axis is tiled and its seams lie
    all on the stride's grid (on) or at least one lies off it."""
    c = Case(*a, tr=True, **kw)
    if grid is not None:
        grid = [grid] if isinstance(grid, tuple) else grid
        c.expect = lambda r: all(bool(seam_phases(c, r, ax)) and (seam_phases(c, r, ax) == {0}) == on for ax, on in grid)
    return c


TRANSPOSED_ROUTES = [
    # ------------------------------------------------------------------------------------------------ float32 1-D
    # (the general kernel is the only 1-D kernel that takes up > 1; "1d-general-single" has its transposed case in ROUTES)
    Route("1d-general-running-sum", {}, _1d(pers_nb=0, accumulate=1, chunk_launches=0, wide=0, dense=0, nseg=1), [
        _t(2, 9, 6, (1500,), (33,), s=2, p=16, grads=True, public=True, grid=(0, True)),
        _t(2, 9, 6, (1500,), (33,), s=2, p=15, op=1, grid=(0, False)),
        _t(3, 12, 8, (1000,), (31,), s=3, p=4, d=2, op=2),
        _t(2, 32, 16, (900,), (17,), s=2, p=3, op=1, g=2),
    ]),
    Route("1d-chunk-launches", {}, _1d(chunk_launches=1, pers_nb=0), [
        _t(2, 20, 6, (2000,), (700,), s=2, p=100, d=3, op=1, grads=True, public=True, grid=(0, False)),
        _t(1, 9, 4, (1500,), (1101,), s=2, d=2, grid=(0, True)),
        _t(2, 34, 12, (1500,), (2101,), s=2, p=51, op=1, g=2, grid=(0, False)),
    ]),
    Route("1d-segments", {}, lambda r: _1d(diag=0)(r) and r["nseg"] > 1, [
        _t(2, 8, 8, (6000,), (5000,), s=2, grads=True, public=True, grid=(0, False)),
        _t(2, 16, 16, (3000,), (5000,), s=2, p=1, op=1, g=2, grid=(0, True)),
        _t(1, 4, 6, (4000,), (3000,), s=2, p=51, d=2, op=1, grid=(0, False)),
        _t(2, 12, 8, (3000,), (4500,), s=3, p=100, op=2),
    ]),
    # ------------------------------------------------------------------------------------------------ float32 N-d
    Route("2d-separable-cob2", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=2, Tm=0), [
        _t(5, 2, 2, (30, 200), (5, 5), s=2, p=2, op=1, public=True),
        _t(3, 1, 2, (30, 200), (5, 3), s=2, p=(2, 1)),
        _t(1, 2, 2, (25, 35), (3, 5), s=(2, 3), p=1, op=(1, 2)),
    ]),
    Route("2d-separable-cob4", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=4, Tm=0), [
        _t(5, 3, 4, (30, 200), (5, 5), s=2, p=2, op=1, public=True),
        _t(3, 4, 4, (20, 250), (3, 3), s=(1, 2), p=1),
        _t(1, 3, 4, (17, 23), (4, 2), s=(2, 3), p=(1, 0), op=(1, 2)),
    ]),
    Route("2d-separable-cob8", {"FFTCONV_PLANES": "0"}, _nd(planes=0, cob=8, Tm=0), [
        _t(5, 8, 8, (20, 200), (5, 5), s=2, p=2, op=1, public=True),
        _t(3, 6, 9, (20, 150), (3, 7), s=(1, 2), p=(1, 3), note="cog9"),
        _t(2, 32, 16, (20, 50), (3, 3), s=2, p=1, d=2, op=1, g=2, note="g2"),
        _t(2, 17, 8, (10, 25), (3, 3), s=2, p=1, note="cig17"),
    ]),
    Route("2d-x-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0, Tm=0)(r) and r["nxt"] > 1, [
        _t(2, 4, 4, (30, 300), (3, 7), s=(1, 2), p=(1, 3), public=True, grid=(1, False)),
        _t(2, 4, 4, (30, 300), (3, 7), s=(1, 2), p=(1, 2), op=(0, 1), g=2, grid=(1, True)),
        _t(1, 2, 3, (8, 1700), (3, 65), s=(1, 3), p=(1, 32), op=(0, 2)),
    ]),
    Route("2d-outer-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0, Tm=0)(r) and r["ntiles"] > 1, [
        _t(1, 2, 3, (1000, 9), (40, 3), s=(3, 1), p=(5, 1), d=(2, 1), public=True, grid=(0, False)),
        _t(2, 4, 4, (1200, 20), (65, 3), s=(2, 1), p=(32, 1), op=(1, 0), grid=(0, True)),
        _t(2, 4, 4, (1200, 20), (65, 3), s=(2, 1), p=(31, 1), g=2, grid=(0, False)),
    ]),
    Route("2d-colz-b1", {"FFTCONV_PLANES": "2"}, _nd(planes=2), [
        _t(1, 8, 8, (50, 100), (5, 5), s=2, p=2, op=1, public=True),
        _t(1, 6, 5, (32, 65), (3, 3), s=2, p=1),
        _t(1, 8, 16, (35, 50), (5, 3), s=(2, 3), p=(2, 1), op=(1, 2)),
    ]),
    Route("2d-colz-b2", {"FFTCONV_PLANES": "2"}, _nd(planes=2), [
        _t(2, 8, 8, (50, 100), (5, 5), s=2, p=2, op=1, public=True),
        _t(3, 6, 5, (32, 65), (3, 3), s=2, p=1),
        _t(5, 16, 8, (20, 48), (7, 3), s=(2, 3), p=(3, 1), op=(1, 2), g=2),
    ]),
    Route("3d-separable-y-tiles", {"FFTCONV_PLANES": "0"}, lambda r: _nd(planes=0)(r) and r["nyt"] > 1, [
        _t(1, 2, 3, (8, 260, 20), (3, 7, 3), s=(1, 2, 1), p=(1, 3, 1), d=(1, 2, 1), public=True, grid=(1, False)),
        _t(2, 4, 4, (6, 300, 10), (3, 5, 3), s=(1, 2, 1), p=(1, 2, 1), op=(0, 1, 0), g=2, grid=(1, True)),
    ]),
    Route("3d-planes-untiled", {}, lambda r: _nd(planes=1)(r) and r["nxt"] * r["nyt"] == 1, [
        _t(2, 8, 8, (10, 20, 20), (3, 3, 3), s=2, p=1, op=1, public=True),
        _t(1, 8, 16, (15, 33, 16), (5, 3, 2), s=(2, 1, 3), p=(2, 1, 0), op=(1, 0, 2)),
        _t(3, 6, 6, (17, 16, 20), (2, 3, 3), s=(1, 2, 1), p=1),
    ]),
    Route("3d-planes-tiled", {}, lambda r: _nd(planes=1, Tx=64, Tm=64)(r) and r["nxt"] * r["nyt"] > 1, [
        _t(2, 8, 8, (20, 50, 65), (3, 5, 5), s=(1, 2, 2), p=2, op=(0, 1, 1), public=True, grid=[(1, True), (2, True)]),
        _t(2, 8, 8, (20, 50, 65), (3, 5, 5), s=(1, 2, 2), p=(2, 1, 1), grid=[(1, False), (2, False)]),
        _t(1, 8, 16, (30, 35, 30), (5, 3, 7), s=(1, 2, 3), p=(2, 1, 3), op=(0, 1, 2)),
    ]),
    # ------------------------------------------------------------------------------------------------ float64
    Route("f64-direct", {}, _f64("f64_direct"), [
        _t(2, 3, 4, (10, 15), (3, 3), s=2, p=1, op=1, f64=True, public=True, grads=True),
        _t(3, 4, 6, (250,), (9,), s=2, p=4, d=2, g=2, f64=True),
        _t(2, 2, 2, (4, 5, 6), (2, 3, 2), s=2, p=1, op=1, f64=True),
    ]),
    Route("f64-nd-nb1", {}, _f64("f64_fft_nd", nb=1), [
        _t(2, 4, 9, (15, 20), (7, 7), s=2, p=3, op=1, f64=True, public=True, grads=True, note="cog9", grid=(0, False)),
        _t(1, 4, 2, (15, 20), (7, 7), s=2, p=2, f64=True, grid=(1, True)),
        _t(2, 4, 6, (6, 7, 5), (3, 3, 3), s=2, p=1, op=1, f64=True),
    ]),
    Route("f64-nd-nb2", {}, _f64("f64_fft_nd", nb=2), [
        _t(3, 4, 3, (15, 20), (7, 7), s=2, p=3, op=1, f64=True, public=True, grads=True, grid=(1, False)),
        _t(2, 9, 4, (11, 17), (7, 7), s=(2, 3), p=(3, 2), f64=True),
        _t(2, 6, 4, (5, 6, 7), (3, 3, 4), s=2, p=1, op=1, g=2, f64=True),
    ]),
    Route("f64-nd-nb4", {}, _f64("f64_fft_nd", nb=4), [
        _t(5, 4, 2, (15, 20), (7, 7), s=2, p=3, op=1, f64=True, public=True, grads=True, note="rem1"),
        _t(6, 4, 2, (13, 16), (7, 7), s=2, p=2, f64=True, note="rem2", grid=(0, True)),
        _t(7, 6, 2, (5, 6, 7), (3, 3, 3), s=2, p=1, op=1, f64=True, note="rem3"),
        _t(4, 4, 4, (10, 11), (7, 8), s=2, p=1, op=1, g=2, f64=True, note="g2"),
    ]),
    Route("f64-2048-tiles", {}, lambda r: (r["kind"] == "f64_fft_1d" and r["T"] == 2048) or
          (r["kind"] == "f64_fft_nd" and 2048 in (r["t0"], r["t1"], r["t2"])), [
        _t(2, 2, 3, (2500,), (601,), s=2, p=10, op=1, f64=True, public=True, grads=True, grid=(0, True)),
        _t(2, 2, 3, (2500,), (601,), s=2, p=11, f64=True, grid=(0, False)),
        _t(1, 1, 2, (10, 1250), (3, 513), s=(1, 2), p=(1, 0), d=(1, 2), op=(0, 1), f64=True, grid=(1, True)),
        _t(1, 1, 2, (10, 1250), (3, 513), s=(1, 2), p=(1, 1), d=(1, 2), f64=True, grid=(1, False)),
    ]),
]

# The batch-sharing, wide, dense, depthwise and block-diagonal 1-D kernels refuse strided transposed plans (the
# d.stride[0] == 1 conditions of csrc/host_1d.cpp: a tile of theirs starts anywhere on the spread row), so TRANSPOSED_ROUTES
# has no entry for them.  Under each route's knobs the strided plan must land on a general route, and the stride-1 plan of
# the same shape on the route itself ((name, knobs, strided transposed case, the route's own predicate)).
GENERAL_1D = _1d(pers_nb=0, wide=0, dense=0, diag=0, bd_gs=0)
TRANSPOSED_REFUSED = [
    ("batch-sharing-nb2", {"FFTCONV_PERS": "2"}, _t(3, 8, 8, (1000,), (129,), s=2, op=1), _1d(pers_nb=2)),
    ("batch-sharing-nb4", {"FFTCONV_PERS": "4"}, _t(5, 8, 8, (1000,), (129,), s=2, op=1), _1d(pers_nb=4)),
    ("wide", {}, _t(3, 16, 8, (2500,), (100,), s=2, p=16, op=1), _1d(wide=1)),
    ("dense", {"FFTCONV_DENSE": "2"}, _t(4, 64, 64, (4500,), (129,), s=2, p=64, op=1), _1d(dense=1)),
    ("depthwise", {}, _t(3, 24, 24, (2500,), (33,), g=24, s=2, p=5, op=1), _1d(diag=1)),
    ("block-diagonal-gs2", {"FFTCONV_PERS": "2"}, _t(4, 16, 16, (5000,), (257,), g=8, s=2, op=1), _1d(bd_gs=2)),
    ("block-diagonal-gs4", {"FFTCONV_PERS": "2"}, _t(3, 32, 32, (4500,), (129,), g=8, s=2, p=30, op=1), _1d(bd_gs=4)),
]
