// host_1d.cpp -- float32 1-D plans (PlanKind::F32_1D): tile and kernel flavour (general, batch-sharing, wide, dense
// many-channel pipeline), segments of long kernels, dilation as phases, the batch-sharing kernels' work list; the kernel
// transform and the forward of such a plan; the 1-D weight gradient (fc_wgrad1d*).
//
// Planning decides, then builds: decide_route works out everything about one candidate channel layout as a plain value
// (Route1d: no HIP call, nothing written into the plan), plan_1d keeps the first candidate whose route it accepts, and
// build_plan_1d alone writes that route into the plan and allocates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fc_plan.h"

namespace fc {

// The environment knobs of the 1-D planner.  Read at every plan creation (and every weight-gradient geometry), never
// cached: tests and A/B runs change them between two plans of one process.
struct Knobs1d {
  bool pers_set;    // FFTCONV_PERS is set (an empty string counts, with value 0); unset: the planner's own choice
  int pers;         //   0 general kernel only, n force nb = n; 0 when unset
  int ph2;          // FFTCONV_PH2 = 0 / 1 keeps single phases / pairs (default 2: quads where they fit)
  int dense;        // FFTCONV_DENSE = 0 keeps the fused kernels, 2 forces the pipeline (default 1)
  int wide;         // FFTCONV_WIDE = 0 keeps > 8 input channels per group off the batch-sharing work list (default 1)
  bool diag;        // FFTCONV_DIAG = 0: no depthwise / block-diagonal 8 x 8 blocks (forward and weight gradient)
  int dense_slab;   // FFTCONV_DENSE_SLAB: rows per slab of the dense pipeline (testing knob); 0 when unset
};

static Knobs1d read_knobs_1d() {
  auto num = [](const char* e, int unset) { return e ? atoi(e) : unset; };
  const char* pers = getenv("FFTCONV_PERS");
  const char* slab = getenv("FFTCONV_DENSE_SLAB");
  Knobs1d k;
  k.pers_set = pers != nullptr; k.pers = num(pers, 0);
  k.ph2 = num(getenv("FFTCONV_PH2"), 2);
  k.dense = num(getenv("FFTCONV_DENSE"), 1);
  k.wide = num(getenv("FFTCONV_WIDE"), 1);
  k.diag = num(getenv("FFTCONV_DIAG"), 1) != 0;
  k.dense_slab = slab ? std::max(1, atoi(slab)) : 0;
  return k;
}

// What the planner decides for one candidate channel layout: a plain value, copied into the plan by build_plan_1d.
struct Route1d {
  int G, accumulate;            // the channel layout: G blocks of 8 x 8 in a block mode, else the plan's own groups
                                // (set_channel_layout; chunk launches clear its accumulate)
  fc_plan::F1d f;               // its mode (diag, bd_gs), nseg, seg_taps, dense, wide, ph, ph2, slot_tiles, chunk_launches,
                                // pers_nb, pers_items, pers_grid; the sizes and device pointers stay zero
  int64_t kd_plan;              // dilated extent the tiles are planned for (of one segment)
  const TileImpl* tile;
  int V, ntiles;
  std::vector<WorkItem> items;  // work list of the batch-sharing kernels, in launch order
};

// the batch-sharing and wide kernels address x through 32-bit byte offsets
static bool sharing_offsets_fit(const fc_plan& p) {
  return ((int64_t)p.d.in_channels * 3 + p.Cig) * p.d.spatial[0] * 4 < ((int64_t)1 << 32);
}

static bool fast_path_eligible(const fc_plan& p, const Route1d& r) {
  if (p.CB != 8 || r.accumulate || r.f.chunk_launches || p.Cog % 8 != 0 || p.d.stride[0] != 1) return false;   // (a transposed plan with stride 1 is a padded correlation: same kernel)
  if (!sharing_offsets_fit(p)) return false;
  // the kernel stores through a resource over one out-chunk's rows of a batch item (cob * Lout samples) and marks a dead
  // store with bit 31 of its offset: that stays outside only while the rows end below bit 31, a few KB of immediate
  // offsets included (zero padding makes Lout as long as it likes while L stays short)
  if ((int64_t)p.cob * p.out_sp[0] * 4 >= 0x7F000000LL) return false;
  return true;
}

// Joint choice of FFT tile and kernel flavour for 8-channel chunks.  Measured per-workgroup times on
// MI355X (us, phase_profile.py, cfgA-like rows): the general kernel at 2048 / 1024 and the
// batch-sharing kernel at (2048, nb 2), (1024, nb 2), (1024, nb 4); estimated launch time =
// residency rounds x time per workgroup.  Small problems are decided by the rounds, large ones by
// outputs per microsecond.
// Sets r.f.ph and r.f.slot_tiles and returns the tile with the slot count in *nb_out; 0: the cost model decides.
static int choose_fast_path(const fc_plan& p, const Knobs1d& k, int cus, Route1d& r, int* nb_out) {
  const fc_desc& d = p.d;
  const int want = k.pers_set ? k.pers : -1;        // -1 auto, 0 general kernel only, n force nb = n
  const bool fast_ok = want != 0 && fast_path_eligible(p, r);
  const int64_t per_item_units = (int64_t)p.n_ochunks * p.G;
  // {tile, batch items per workgroup (0 = general kernel), resident workgroups per CU, us per workgroup}
  // Launch-time model (round 3, `profiles/r03_planner_sweep.jsonl`: every candidate forced in turn on 12 shapes):
  //   general kernel        est = rounds x t_item, one item per workgroup (t_item: a full round, launch included)
  //   batch-sharing kernel  workgroups run up to two items back to back (grid as build_work_list builds it);
  //                         est = kLaunchUs + sum over waves of workgroups of (items per workgroup x t(occupancy)),
  //                         t(occ) between t_alone (one workgroup on its CU) and t_item (CU full): a 256-thread
  //                         workgroup alone on a CU runs an item in 10.5 us, beside a second one in 14.2
  // The round-2 table priced a batch-sharing workgroup at 15-19.5 us whatever it ran beside and however many items it
  // took: 15-25 % regret wherever fewer workgroups than slots exist or the grid spills into a second wave.
  struct Cand { int T, nb, wgs_per_cu; double t_item, t_alone; };
  const Cand cands[] = {{256, 0, 8, 11.7, 0}, {512, 0, 6, 17.0, 0}, {1024, 0, 4, 25.5, 0}, {2048, 0, 2, 28.9, 0},
                        {2048, 2, 1, 17.3, 17.3}, {2048, 1, 2, 26.0, 13.4}, {1024, 2, 2, 14.2, 10.5}, {1024, 4, 1, 13.3, 13.3}};
  const double kLaunchUs = 4.0;
  double best = 0;
  int best_T = 0, best_nb = 0, best_ph = 1;
  bool best_tiles = false;
  // second round: dilation d as d phases of a virtual batch B*d against the undilated kernel
  const int rounds = (fast_ok && d.dilation[0] > 1 && r.f.nseg == 1) ? 2 : 1;
  for (int round = 0; round < rounds; ++round) {
    const int ph = round ? (int)d.dilation[0] : 1;
    const int64_t Kd = round ? d.kernel[0] : r.kd_plan;
    const int64_t Lfull = (p.Lf[0] + ph - 1) / ph;
    const int64_t B = d.batch * ph;
    for (const Cand& c : cands) {
      if ((round || r.f.diag) && c.nb == 0) continue;  // only the batch-sharing kernel knows phases / depthwise blocks
      if (c.T < Kd || r.accumulate) continue;
      if (c.nb != 0 && !fast_ok) continue;
      if (want > 0 && c.nb != want) continue;
      const int64_t V = c.T - Kd + 1;
      if (V * 4 < c.T) continue;                      // less than a quarter of the tile useful: leave to the cost model
      const int64_t nt = (Lfull + V - 1) / V;
      // fewer batch items than slots: the slots of a work item become consecutive TILES of one batch item
      // (they share the spectrum just the same); measured 1.3-1.6x on batch-1 rows of 2^20 samples
      const bool by_tiles = c.nb > B;
      if (by_tiles && nt < c.nb) continue;
      const int64_t groups_of = by_tiles ? B * ((nt + c.nb - 1) / c.nb) : ((B + std::max(c.nb, 1) - 1) / std::max(c.nb, 1)) * nt;
      const int64_t items = groups_of * per_item_units;
      const int64_t slots = (int64_t)cus * c.wgs_per_cu;
      double est;
      if (c.nb == 0) {
        est = (double)((items + slots - 1) / slots) * c.t_item;
      } else {
        const int64_t grid = std::max<int64_t>((items + 1) / 2, std::min<int64_t>(items, slots));
        const double ipw = (double)items / (double)grid;                 // 1 .. 2 items per workgroup
        auto t_occ = [&](int64_t wgs) {                                  // per item, `wgs` workgroups spread over the CUs
          const int64_t occ = std::min<int64_t>(c.wgs_per_cu, (wgs + cus - 1) / cus);
          return c.wgs_per_cu > 1 ? c.t_alone + (c.t_item - c.t_alone) * (double)(occ - 1) / (double)(c.wgs_per_cu - 1) : c.t_item;
        };
        const int64_t full = grid / slots, rem = grid % slots;
        // (the makespan of a wave is its slowest workgroup: whole items)
        est = kLaunchUs + (double)full * std::ceil(ipw) * c.t_item + (rem ? std::ceil(ipw) * t_occ(rem) : 0.0);
      }
      if (best_T == 0 || est < best) { best = est; best_T = c.T; best_nb = c.nb; best_ph = ph; best_tiles = by_tiles; }
    }
  }
  if (best_T == 0) return 0;                        // general planner (cost model) decides
  *nb_out = best_nb;
  r.f.ph = best_ph;
  r.f.slot_tiles = best_tiles ? 1 : 0;
  return best_T;
}

// Work list of the persistent fused kernel: items of up to NB batch items that share (tile, group,
// out-chunk), largest first; workgroup w takes items w, w+grid, ...  One workgroup per LDS slot.
// nb: the planner's pick (0 = general kernel).  r.f.pers_nb stays 0 when the batch-sharing kernels do not take the route.
static void build_work_list(const fc_plan& p, const Knobs1d& k, int cus, int nb, Route1d& r) {
  const fc_desc& d = p.d;
  if (!r.f.wide && !fast_path_eligible(p, r)) return;
  const fc::TileImpl* t = r.tile;
  const int64_t B = d.batch * r.f.ph;                   // virtual batch (dilation phases)
  if (d.tile_hint && !r.f.wide) nb = k.pers;            // explicit tile: FFTCONV_PERS picks the flavour (default general)
  int wgs_per_cu;
  if (r.f.wide) {
    nb = t->wide_nb;
    wgs_per_cu = std::max(1, (int)((160 * 1024) / t->wide_lds));
  } else {
    if (nb != t->pers_nb[0] && nb != t->pers_nb[1]) nb = 0;
    if (nb == 0) return;
    const int slot = nb == t->pers_nb[0] ? 0 : 1;
    wgs_per_cu = std::max(1, (int)((160 * 1024) / t->pers_lds[slot]));
  }
  // Items: up to nb batch items that share (tile, group, out-chunk), full items first.  When the last
  // residency round would fill less than half of the CUs, its items are split in two so the tail
  // spreads over twice as many CUs (cfgA: 336 pairs on 256 CUs -> 256 pairs + 160 singles).
  std::vector<fc::WorkItem> items;
  const int nfull = (int)(B / nb), rem = (int)(B % nb);
  const int64_t slots = (int64_t)cus * wgs_per_cu;
  const int units = p.n_ochunks * p.G;
  auto is_border = [&](int tile) {
    const int64_t pos = (int64_t)tile * r.V * r.f.ph - p.padl[0];
    return !(p.up[0] == 1 && pos >= 0 && pos + (int64_t)(t->T - 1) * r.f.ph + r.f.ph <= d.spatial[0]);
  };
  if (r.f.slot_tiles) {
    // slots = consecutive tiles of one (virtual) batch item: chunks that touch a border tile go first
    for (int pass = 0; pass < 2; ++pass)
      for (int64_t vb = 0; vb < B; ++vb)
        for (int goc = 0; goc < units; ++goc)
          for (int t0 = 0; t0 < r.ntiles; t0 += nb) {
            const int n = std::min(nb, r.ntiles - t0);
            bool border = false;
            for (int j = 0; j < n; ++j) border |= is_border(t0 + j);
            if ((pass == 0) == border) items.push_back({(int)vb, n, t0, goc});
          }
  } else {
    // border tiles (staged, slower loads) are issued first so they never form the tail of the launch
    for (int pass = 0; pass < 2; ++pass)
      for (int tile = 0; tile < r.ntiles; ++tile) {
        if ((pass == 0) != is_border(tile)) continue;
        for (int goc = 0; goc < units; ++goc)
          for (int c = 0; c < nfull; ++c) items.push_back({c * nb, nb, tile, goc});
      }
  }
  // phase quads (conv1d_pers.hpp PH4): four phases, a multiple of 4 of them per batch item, one full 8 x 8 channel block;
  // FFTCONV_PH2 = 0 / 1 keeps single phases / pairs (A/B runs, tests).  Decided before the tail split: a quad item cannot
  // be halved (a wave owns all four phases of its channel).
  const bool ph_base = r.f.ph > 1 && !r.f.slot_tiles && !r.f.diag && !r.f.wide && r.f.nseg == 1 && nb >= 2 && t->S == 1;
  const bool quads = k.ph2 >= 2 && ph_base && r.f.ph % 4 == 0 && nb == 4 && p.Cig == 8 && p.cob == 8 && p.Cog % 8 == 0 && !r.f.bd_gs;
  if (nb >= 2 && (int64_t)items.size() > slots && !quads) {
    const int64_t tail = (int64_t)items.size() % slots;
    if (tail > 0 && tail <= slots / 2) {
      std::vector<fc::WorkItem> split;
      for (int64_t i = (int64_t)items.size() - tail; i < (int64_t)items.size(); ++i) {
        const fc::WorkItem w = items[i];
        const int h = w.nbc / 2;
        if (h == 0) { split.push_back(w); continue; }
        split.push_back({w.b0, h, w.tile, w.goc});
        if (r.f.slot_tiles) split.push_back({w.b0, w.nbc - h, w.tile + h, w.goc});
        else split.push_back({w.b0 + h, w.nbc - h, w.tile, w.goc});
      }
      items.resize(items.size() - tail);
      items.insert(items.end(), split.begin(), split.end());
    }
  }
  if (rem && !r.f.slot_tiles)
    for (int tile = 0; tile < r.ntiles; ++tile)
      for (int goc = 0; goc < units; ++goc) items.push_back({nfull * nb, rem, tile, goc});
  if (items.size() > 0x7fffffffu) return;
  r.f.pers_items = (int)items.size();
  // up to two items per workgroup (the second one's input is prefetched): item i and i + grid
  r.f.pers_grid = (int)std::max<int64_t>((r.f.pers_items + 1) / 2, std::min<int64_t>(r.f.pers_items, slots));
  if (r.f.wide) r.f.pers_grid = r.f.pers_items;         // one item per workgroup
  r.items = std::move(items);
  r.f.pers_nb = nb;
  // phases in pairs: an even number of phases, slots = batch items (so slots 2j, 2j+1 are neighbouring phases of one
  // batch item), plain dense-block kernel on a P*P tile; quads (above) take precedence
  r.f.ph2 = quads ? 2 : ((k.ph2 != 0 && ph_base && r.f.ph % 2 == 0) ? 1 : 0);
}

static size_t group_spectrum_bytes(const fc_plan& p, const fc::TileImpl* t) {
  return (size_t)p.Cog_pad * (p.Cig_pad / 2) * (t->T / 2) * sizeof(fc::f4);
}

// The route of a plan with the axis geometry (as fc_api.cpp filled it) and the channel layout of `p`, in the given mode of
// that layout.  Calls nothing of HIP and leaves `p` as it is.
static int decide_route(const fc_plan& p, int diag, int bd_gs, const Knobs1d& k, int cus, Route1d& r) {
  const fc_desc& d = p.d;
  r = Route1d{};
  r.G = p.G; r.accumulate = p.accumulate; r.f.diag = diag; r.f.bd_gs = bd_gs; r.f.ph = 1;
  // Long kernels run in segments of taps: segment j is the convolution with taps [j*Ks, (j+1)*Ks) read
  // j*Ks*dilation samples further into the row, later segments add into y.  This lifts the 4096-point tile
  // limit on the dilated extent and keeps 8-channel shapes on the batch-sharing kernel beyond its 2048 tile.
  r.f.nseg = 1; r.f.seg_taps = (int)d.kernel[0]; r.kd_plan = p.kd[0];
  {
    const bool sharing_shape = p.CB == 8 && p.Cog % 8 == 0 && d.stride[0] == 1;
    const bool want_seg = p.kd[0] > 4096 || (sharing_shape && p.kd[0] > 1537 && !d.tile_hint);
    if (want_seg) {
      const int64_t ks = std::max<int64_t>(1, 1024 / d.dilation[0] + 1);       // (ks - 1) * dilation + 1 <= 1025
      r.f.seg_taps = (int)std::min<int64_t>(ks, d.kernel[0]);
      r.f.nseg = (int)((d.kernel[0] + r.f.seg_taps - 1) / r.f.seg_taps);
      r.kd_plan = (int64_t)(r.f.seg_taps - 1) * d.dilation[0] + 1;
    }
  }
  const int64_t L = d.spatial[0], Kd = r.kd_plan, Lfull = p.Lf[0];
  if (L * (int64_t)std::max(p.Cig, 1) * 4 >= (int64_t)1 << 32)
    return fail(FC_ERR_UNSUPPORTED, "1-D signal too long for 32-bit buffer offsets (Cin/groups * L * 4 must be < 4 GiB)");

  const int NPI = p.CB / 2;
  const size_t lds_cap = 160 * 1024;
  const fc::TileImpl* best = nullptr;
  double best_cost = 0;
  int ntl;
  auto tiles = all_tiles(&ntl);
  int forced_tile = d.tile_hint;
  int nb_choice = 0;                                    // choose_fast_path's pick (0 = general kernel)
  {
    // 16 or more channels per group on BOTH sides, stride 1, kernel within the 1024 tile: transforms and contraction
    // in separate launches, the contraction as one real GEMM per frequency bin on the matrix pipe (dense1d.hpp).
    // FFTCONV_DENSE=0 keeps the fused kernels (A/B runs).
    // Measured against the fused kernels (scripts/dense_check.py, us): 128->96 M = 30 rows 58 / 175; 32->32 M = 144
    // 50 / 84; 64->64 M = 152 91 / 150; but (first build) 24->40 M = 18 44 / 33, 16->24 x 2 groups M = 26 41 / 27,
    // 16->16 M = 2 31 / 23: three launches need work to amortise -- at least 32 channels a side and 64 K row-channel
    // products.  FFTCONV_DENSE=2 forces the pipeline for every shape it can run (tests).
    const int64_t Kd_d = p.kd[0];
    const int dT = Kd_d <= 769 ? 1024 : 2048;             // (at least a quarter of the tile valid)
    const fc::TileImpl* dt = find_tile(dT);
    const int64_t Vd = std::max<int64_t>(1, dT + 1 - Kd_d);
    const int64_t Md = d.batch * ((p.Lf[0] + Vd - 1) / Vd);
    const bool pays = k.dense == 2 || (p.Cig >= 32 && p.Cog >= 32 && Md * p.Cig * p.Cog >= 65536);
    if (k.dense && pays && dt && dt->dense && r.f.nseg == 1 && p.CB == 8 && p.Cig >= 16 && p.Cog >= 16 && d.stride[0] == 1 &&
        p.up[0] == 1 && !r.f.diag && !r.f.bd_gs && Kd <= 1537 && (!forced_tile || forced_tile == dT) &&
        (int64_t)p.Cig * d.spatial[0] * 4 < ((int64_t)1 << 32)) {
      // 32-bit offsets of the pipeline: dense_inv marks dead stores with bit 31 of an offset into one group's output rows
      // (Cog * Lout * 4 bytes), and the slab resources / bin strides are 32-bit too (a slab row block of at least 128
      // rows x NF bins x max(Kc, Nc) channels).  Shapes beyond either limit stay with the fused kernels.
      const int64_t NFd = dT / 2 + 1;
      const int64_t rows_min = std::min<int64_t>(Md, 128);
      const bool out_ok = (int64_t)p.Cog * p.out_sp[0] * 4 < ((int64_t)1 << 31);
      const bool slab_ok = NFd * rows_min * std::max(p.Cig_pad, p.Cog_pad) * 8 < ((int64_t)1 << 32);
      if (out_ok && slab_ok) {
        r.f.dense = 1;
        forced_tile = dT;
      }
    }
  }
  if (!r.f.dense) {
    // more than 8 input channels per group, whole out-chunks, stride 1: the register-accumulating
    // batch-sharing kernel (1024 or 2048 tile, whichever keeps at least a quarter of the tile valid).
    // Short kernels stay with the general kernel and its small tiles (measured: 16->16, k = 33, L = 4096:
    // 24.6 us there vs 29.1 us here; k = 129 ... 1025: 2.0-2.5x faster here).
    if (k.wide && r.f.nseg == 1 && p.CB == 8 && r.accumulate && p.Cog % 8 == 0 && d.stride[0] == 1 && d.batch >= 2 &&
        sharing_offsets_fit(p)) {
      const int wt = Kd < 97 ? 0 : (Kd <= 768 ? 1024 : (Kd <= 1536 ? 2048 : 0));
      if (wt && (!forced_tile || forced_tile == wt) && find_tile(wt) && find_tile(wt)->wide_nb) {
        r.f.wide = 1;
        forced_tile = wt;
      }
    }
  }
  if (r.f.wide || r.f.dense) {
    // tile fixed above
  } else if (!forced_tile) {
    forced_tile = choose_fast_path(p, k, cus, r, &nb_choice);
  } else if (d.dilation[0] > 1 && fast_path_eligible(p, r) && k.pers_set && k.pers > 0) {
    r.f.ph = (int)d.dilation[0];           // explicit tile + explicit flavour: dilation as phases
  }
  // dilation as phases: the kernel seen by a tile is the undilated one, rows are 1/ph as long
  const int64_t Kd_t = r.f.ph > 1 ? d.kernel[0] : Kd;
  const int64_t Lfull_t = r.f.ph > 1 ? (Lfull + r.f.ph - 1) / r.f.ph : Lfull;
  for (int attempt = 0; attempt < 2 && !best; ++attempt) {
    if (attempt == 1) {
      // No tile holds the kernel together with the second (running-sum) LDS region of a multi-chunk plan:
      // launch the general kernel once per input chunk instead, chunks after the first adding into y.
      if (!r.accumulate || r.f.wide || r.f.dense || forced_tile) break;
      r.accumulate = 0;
      r.f.chunk_launches = 1;
    }
    for (int i = 0; i < ntl; ++i) {
      const fc::TileImpl* t = tiles[i];
      if (forced_tile && t->T != forced_tile) continue;
      if (t->T < Kd_t) continue;
      const size_t lds = r.f.wide ? t->wide_lds : (r.f.dense ? 0 : (size_t)(r.accumulate ? 2 : 1) * NPI * t->lseq * sizeof(fc::f2));
      if (lds > lds_cap) continue;
      if (t->NT / (t->P * t->S) < NPI) continue;
      const int64_t V = t->T - Kd_t + 1;
      const int64_t nt = (Lfull_t + V - 1) / V;
      // work model: FFT passes + channel mix per tile; the largest tile runs one
      // workgroup per CU (LDS), which costs latency hiding
      double cost = (double)nt * t->T * (2.0 * std::log2((double)t->T) + 4.0 + p.CB);
      // measured (cfgD, MI355X): one 512-thread workgroup per CU and the four-lane split cost the
      // 4096 tile ~1.7x per sample of tile; it only wins when the kernel is nearly as long as 2048
      if (lds > 80 * 1024) cost *= 1.7;
      if (!best || cost < best_cost) { best = t; best_cost = cost; }
    }
  }
  if (!best) {
    if (d.tile_hint) return fail(FC_ERR_INVALID, "tile_hint %d is not usable for this problem", d.tile_hint);
    if (Kd <= 4096)
      return fail(FC_ERR_UNSUPPORTED, "dilated kernel extent %lld needs the 4096-point tile, which cannot hold the running "
                  "sums of more than 8 input channels per group (%d here)", (long long)Kd, p.Cig);
    return fail(FC_ERR_UNSUPPORTED, "dilated kernel extent %lld exceeds the largest FFT tile (4096)", (long long)Kd);
  }
  r.tile = best;
  r.V = (int)(best->T - Kd_t + 1);
  r.ntiles = (int)((Lfull_t + r.V - 1) / r.V);
  if (group_spectrum_bytes(p, best) >= ((size_t)1 << 32))
    return fail(FC_ERR_UNSUPPORTED, "kernel spectrum of one group exceeds 4 GiB");
  if (!r.f.dense) build_work_list(p, k, cus, nb_choice, r);
  if (r.f.ph > 1 && r.f.pers_nb == 0)
    return fail(FC_ERR_INVALID, "internal: phase plan without the batch-sharing kernel");
  return FC_OK;
}

// Writes the chosen route into the plan, sizes its LDS, kernel spectrum and workspace, and makes the device tables: the
// twiddles of its tile and the work list.  The only allocating step of plan_1d.
static int build_plan_1d(fc_plan* p, const Route1d& r, const Knobs1d& k, int cus) {
  if (r.f.diag || r.f.bd_gs) set_channel_layout(p, r.G, 8, 8);
  p->accumulate = r.accumulate;
  p->f1d = r.f;
  const fc::TileImpl* best = r.tile;
  p->tile = best; p->V = r.V; p->ntiles = r.ntiles; p->Lfull = p->Lf[0];
  const int NPI = p->CB / 2;
  p->f1d.lds_conv = (size_t)(p->accumulate ? 2 : 1) * NPI * best->lseq * sizeof(fc::f2);
  p->f1d.lds_spec = (size_t)(best->NT / (best->P * best->S)) * best->lseq * sizeof(fc::f2);
  p->f1d.seg_spectrum_bytes = r.f.diag ? (size_t)(round_up(p->d.in_channels, 8) / 2) * (best->T / 2) * sizeof(fc::f4)
                                     : group_spectrum_bytes(*p, best) * (size_t)p->G;
  p->spectrum_bytes = p->f1d.seg_spectrum_bytes * (size_t)r.f.nseg;
  p->workspace_bytes = 0;
  int rc = get_twiddles(best, &p->tw);
  if (rc != FC_OK) return rc;
  if (r.f.dense) {
    // spectrum: bin-major complex matrices; workspace: one slab of X and Y rows (<= 192 MiB), or the fused-layout
    // spectrum while the kernel is being transformed
    const size_t NF = (size_t)best->T / 2 + 1;
    const size_t fused_bytes = p->spectrum_bytes;      // the kernel spectrum before the bin-major re-layout
    p->spectrum_bytes = (size_t)p->G * NF * p->Cig_pad * p->Cog_pad * sizeof(fc::f2);
    p->f1d.seg_spectrum_bytes = p->spectrum_bytes;
    const int64_t M = p->d.batch * (int64_t)p->ntiles;
    const size_t row_bytes = (size_t)p->G * NF * (size_t)(p->Cig_pad + p->Cog_pad) * sizeof(fc::f2);
    int64_t slab = (int64_t)(((size_t)192 << 20) / row_bytes) / 128 * 128;
    slab = std::max<int64_t>(128, slab);
    // (32-bit offsets inside a slab: NF * rows * channels * 8 bytes per side; decide_route admitted the shape for 128 rows)
    while (slab > 128 && (int64_t)NF * slab * std::max(p->Cig_pad, p->Cog_pad) * 8 >= ((int64_t)1 << 32)) slab -= 128;
    if (k.dense_slab) slab = k.dense_slab;             // testing knob: rows per slab
    p->f1d.dense_mslab = (int)std::min<int64_t>(M, slab);
    p->f1d.dense_cus = cus;
    p->workspace_bytes = std::max(row_bytes * (size_t)p->f1d.dense_mslab, fused_bytes);
    return FC_OK;
  }
  if (r.f.pers_nb) {
    FC_HIP_SETUP(hipMalloc(&p->f1d.d_items, r.items.size() * sizeof(fc::WorkItem)));
    FC_HIP_SETUP(hipMemcpy(p->f1d.d_items, r.items.data(), r.items.size() * sizeof(fc::WorkItem), hipMemcpyHostToDevice));
  }
  return FC_OK;
}

// The candidate layouts in turn, the first acceptable route built.  Groups of 2 or 4 channels and depthwise rows
// (groups == Cin == Cout >= 5), stride 1, run on the batch-sharing kernel as blocks of 8 x 8 channels; when that kernel
// does not take the blocks the plain grouped layout is planned.
int plan_1d(fc_plan* p) {
  const fc_desc& d = p->d;
  const Knobs1d k = read_knobs_1d();
  int cus = 256;
  if (!current_device_cus(&cus)) return fail(FC_ERR_HIP, "cannot query the current device");
  Route1d r;
  auto blocks_taken = [&](int G, int diag, int bd_gs) {      // by the batch-sharing kernel, as G blocks of 8 x 8 channels
    fc_plan q = *p;                                          // (a candidate: the caller's plan stays as it is)
    set_channel_layout(&q, G, 8, 8);
    return decide_route(q, diag, bd_gs, k, cus, r) == FC_OK && r.f.pers_nb != 0;
  };
  const bool try_blocks = k.diag && d.stride[0] == 1 && !(d.tile_hint && !k.pers_set);
  // groups of 2 or 4 channels (in == out per group): 8 / gs of them form one dense 8 x 8 block whose
  // cross-group spectrum entries are zero -- the batch-sharing kernel runs it as is
  const int64_t gs = d.in_channels / d.groups;
  if (try_blocks && (gs == 2 || gs == 4) && d.out_channels / d.groups == gs && d.groups % (8 / gs) == 0 &&
      blocks_taken((int)(d.groups * gs / 8), 0, (int)gs))
    return build_plan_1d(p, r, k, cus);
  // depthwise rows: blocks of 8 channels with a per-channel mix (the last block may be partly empty: the kernel masks it)
  if (try_blocks && d.groups == d.in_channels && d.groups == d.out_channels && d.groups >= 5 &&
      blocks_taken((int)((d.groups + 7) / 8), 1, 0))
    return build_plan_1d(p, r, k, cus);
  const int rc = decide_route(*p, 0, 0, k, cus, r);         // the plain grouped layout, as fc_api.cpp laid it out
  return rc != FC_OK ? rc : build_plan_1d(p, r, k, cus);
}

int transform_kernel_1d(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st) {
  fc::Spec1dArgs a;
  a.w = weight;
  a.wspec = (fc::f4*)w_hat;
  a.twA = p.tw.twA;
  a.twB = p.tw.twB;
  a.G = p.G; a.Cig = p.Cig; a.Cog = p.Cog; a.Cig_pad = p.Cig_pad; a.Cog_pad = p.Cog_pad;
  if (p.f1d.diag) {   // depthwise: (C, 1, K) read as one output row over C inputs -> [C/2 pairs][T/2] float4
    a.G = 1; a.Cog = 1; a.Cog_pad = 1; a.Cig = (int)p.d.in_channels; a.Cig_pad = (int)round_up(p.d.in_channels, 8);
  }
  a.gs = p.f1d.bd_gs;
  a.dil = p.f1d.ph > 1 ? 1 : (int)p.d.dilation[0];
  a.nseq = a.G * a.Cog_pad * (a.Cig_pad / 2);
  a.transposed = p.d.transposed;
  a.Krow = (int)p.d.kernel[0];
  {
    const unsigned long long wb = 4ull * (unsigned long long)(p.d.transposed ? p.d.in_channels : p.d.out_channels) *
                                  (unsigned long long)((p.d.transposed ? p.d.out_channels : p.d.in_channels) / p.d.groups) * (unsigned long long)p.d.kernel[0];
    a.w_bytes = wb < 0x7F000000ull ? (unsigned)wb : 0u;   // (dead offsets are bit 31 minus at most a few KB: they must stay outside)
  }
  const int per_wg = p.tile->NT / (p.tile->P * p.tile->S);
  const int grid = (a.nseq + per_wg - 1) / per_wg;
  if (p.f1d.dense) {
    // transform into the scratch area in the fused kernels' layout, then re-lay bin-major for the GEMM
    a.k0 = 0; a.K = (int)p.d.kernel[0]; a.wspec = (fc::f4*)workspace;
    FC_HIP(p.tile->spec1d(a, grid, p.f1d.lds_spec, st));
    fc::DenseSpecArgs ds;
    ds.wspec = (const fc::f4*)workspace; ds.Hd = (fc::f2*)w_hat; ds.G = p.G; ds.Kc = p.Cig_pad; ds.Nc = p.Cog_pad; ds.T = p.tile->T;
    FC_HIP(p.tile->dense_spec(ds, st));
    return FC_OK;
  }
  for (int j = 0; j < p.f1d.nseg; ++j) {
    a.k0 = j * p.f1d.seg_taps;
    a.K = std::min(p.f1d.seg_taps, (int)p.d.kernel[0] - a.k0);
    a.wspec = (fc::f4*)((char*)w_hat + (size_t)j * p.f1d.seg_spectrum_bytes);
    FC_HIP(p.tile->spec1d(a, grid, p.f1d.lds_spec, st));
  }
  return FC_OK;
}

int forward_1d(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
               hipStream_t st, void* stamps) {
  if (p.f1d.dense) {
    fc::DenseArgs a{};
    const size_t NF = (size_t)p.tile->T / 2 + 1;
    a.x = x; a.y = y; a.bias = p.d.has_bias ? bias : nullptr; a.Hd = (const fc::f2*)w_hat; a.io = p.io;
    a.twA = p.tw.twA; a.twB = p.tw.twB;
    a.B = (int)p.d.batch; a.Cin = (int)p.d.in_channels; a.Cout = (int)p.d.out_channels; a.G = p.G;
    a.Cig = p.Cig; a.Cog = p.Cog; a.Kc = p.Cig_pad; a.Nc = p.Cog_pad;
    a.L = (int)p.d.spatial[0]; a.pad = p.padl[0]; a.pad_mode = p.d.padding_mode;
    a.V = p.V; a.ntiles = p.ntiles; a.Lfull = p.Lfull; a.Lout = (int)p.out_sp[0];
    a.cus = p.f1d.dense_cus;
    const int64_t M = p.d.batch * (int64_t)p.ntiles;
    for (int64_t m0 = 0; m0 < M; m0 += p.f1d.dense_mslab) {
      a.m0 = (int)m0; a.mcount = (int)std::min<int64_t>(p.f1d.dense_mslab, M - m0);
      a.X = (fc::f2*)workspace;
      a.Y = a.X + (size_t)p.G * NF * (size_t)a.mcount * (size_t)a.Kc;
      FC_HIP(p.tile->dense(0, a, st));
      FC_HIP(p.tile->dense(1, a, st));
      FC_HIP(p.tile->dense(2, a, st));
    }
    return FC_OK;
  }
  fc::Conv1dArgs a;
  a.x = x; a.wspec = (const fc::f4*)w_hat; a.bias = p.d.has_bias ? bias : nullptr; a.y = y;
  a.twA = p.tw.twA; a.twB = p.tw.twB;
  a.B = (int)p.d.batch; a.Cin = (int)p.d.in_channels; a.Cout = (int)p.d.out_channels; a.G = p.G;
  a.Cig = p.Cig; a.Cog = p.Cog; a.Cig_pad = p.Cig_pad; a.Cog_pad = p.Cog_pad; a.cob = p.cob; a.n_ochunks = p.n_ochunks;
  a.L = (int)p.d.spatial[0]; a.pad = p.padl[0]; a.pad_mode = p.d.padding_mode; a.up = p.up[0]; a.ph = p.f1d.ph; a.slot_tiles = p.f1d.slot_tiles; a.diag = p.f1d.diag;
  a.ph2 = p.f1d.ph2;
  a.Kd = (int)p.kd[0]; a.V = p.V; a.ntiles = p.ntiles; a.Lfull = p.Lfull; a.Lout = (int)p.out_sp[0];
  a.stride = p.ostride[0]; a.accumulate = p.accumulate;
  a.ic_begin = 0; a.ic_end = p.Cig_pad / p.CB; a.add_out = 0;
  a.stamps = (unsigned long long*)stamps;
  a.segmented = p.f1d.nseg > 1; a.pos_shift = 0;
  a.io = p.io;
  const int64_t grid = (int64_t)a.B * a.ntiles * a.n_ochunks * a.G;     // of the general kernel
  if (!p.f1d.pers_nb && grid > 0x7fffffff) return fail(FC_ERR_UNSUPPORTED, "grid too large");
  if (p.f1d.chunk_launches) {                                           // (the general kernel, one segment)
    const int n_ichunks = p.Cig_pad / p.CB;
    for (int ic = 0; ic < n_ichunks; ++ic) {
      a.ic_begin = ic; a.ic_end = ic + 1; a.add_out = ic > 0;
      if (ic > 0) a.bias = nullptr;
      FC_HIP(p.tile->conv1d(p.CB, a, (int)grid, p.f1d.lds_conv, st));
    }
    return FC_OK;
  }
  fc::Conv1dPersArgs pa;                                                // (the batch-sharing kernels: a plus the work list)
  pa.items = p.f1d.d_items; pa.n_items = p.f1d.pers_items;
  for (int j = 0; j < p.f1d.nseg; ++j) {
    a.pos_shift = j * p.f1d.seg_taps * (int)p.d.dilation[0];
    a.wspec = (const fc::f4*)((const char*)w_hat + (size_t)j * p.f1d.seg_spectrum_bytes);
    a.add_out = j > 0;
    if (j > 0) a.bias = nullptr;
    pa.c = a;
    if (p.f1d.wide) FC_HIP(p.tile->conv1d_wide(pa, p.f1d.pers_grid, st));
    else if (p.f1d.pers_nb) FC_HIP(p.tile->conv1d_pers(p.f1d.pers_nb, pa, p.f1d.pers_grid, st));
    else FC_HIP(p.tile->conv1d(p.CB, a, (int)grid, p.f1d.lds_conv, st));
  }
  return FC_OK;
}

}  // namespace fc

// ---- 1-D weight gradient
using namespace fc;

namespace {
struct WgradGeom {
  const fc::TileImpl* t;
  int kd_seg, seg_taps, nseg, V, ntiles, nob, nib, Cig, Cog, n_items, ipw, slices, pad, diag, Lout;
};
int wgrad_geometry(const fc_desc& d, WgradGeom* g) {
  const Knobs1d k = read_knobs_1d();             // read per call, like the plan-creation knobs (not frozen at first use)
  // (float16 / bfloat16 x and dY: the float32 geometry -- same slices, segments and kernel -- with 16-bit loads)
  if (d.dtype != FC_F32 && d.dtype != FC_F16 && d.dtype != FC_BF16) return 0;
  if (d.ndim != 1 || d.transposed || d.stride[0] < 1 || d.stride[0] > 64 || d.groups < 1) return 0;
  if (d.batch < 1 || d.in_channels % d.groups || d.out_channels % d.groups) return 0;
  const int64_t Cig = d.in_channels / d.groups, Cog = d.out_channels / d.groups;
  if (Cig > 64 || Cog > 64) return 0;      // every 4 x 4 channel block repeats the transforms of its rows: beyond this the plan path wins
  const int64_t kd = (d.kernel[0] - 1) * d.dilation[0] + 1;
  const fc::TileImpl* t = find_tile(1024);
  if (!t || !t->wgrad1d || d.padding[0] < 0 || d.dilation[0] > 512) return 0;
  if (d.spatial[0] + 2 * d.padding[0] - kd < 0) return 0;
  const int64_t Lout = (d.spatial[0] + 2 * d.padding[0] - kd) / d.stride[0] + 1;
  const int64_t Lext = (Lout - 1) * d.stride[0] + 1;       // the gradient row spread over the stride's grid
  if (d.padding_mode == FC_PAD_REFLECT && d.padding[0] >= d.spatial[0]) return 0;
  if (d.padding_mode == FC_PAD_CIRCULAR && d.padding[0] > d.spatial[0]) return 0;
  if ((int64_t)d.batch * d.in_channels * d.spatial[0] * 4 >= ((int64_t)1 << 32) ||
      (int64_t)d.batch * d.out_channels * Lout * 4 >= ((int64_t)1 << 32)) return 0;
  // the lags of one launch fit half a tile; longer kernels run in segments of taps (x read further in)
  const int64_t ks = std::min<int64_t>(d.kernel[0], kd <= 768 ? d.kernel[0] : 512 / d.dilation[0] + 1);
  const int64_t kd_seg = (ks - 1) * d.dilation[0] + 1;
  const int64_t nseg = (d.kernel[0] + ks - 1) / ks;
  if (nseg > 64) return 0;
  const int64_t V = (t->T - kd_seg + 1) / d.stride[0] * d.stride[0];      // tiles start on the stride's grid
  if (V < 1) return 0;
  const int64_t ntiles = (Lext + V - 1) / V, n_items = (int64_t)d.batch * ntiles;
  if (n_items > 0x3fffffff) return 0;
  int cus = 256;
  if (!current_device_cus(&cus)) return 0;
  g->diag = k.diag && d.groups == d.in_channels && d.groups == d.out_channels && d.groups % 8 == 0 &&
            t->wgrad1d_diag != nullptr;
  const int nb = g->diag ? 1 : t->wgrad_nb;
  g->t = t; g->kd_seg = (int)kd_seg; g->seg_taps = (int)ks; g->nseg = (int)nseg; g->V = (int)V; g->ntiles = (int)ntiles;
  g->Cig = (int)Cig; g->Cog = (int)Cog;
  g->nob = (int)(Cog + 3) / 4; g->nib = (int)(Cig + 3) / 4; g->n_items = (int)n_items; g->pad = (int)d.padding[0]; g->Lout = (int)Lout;
  const int64_t types = g->diag ? d.groups / 8 : (int64_t)d.groups * g->nob * g->nib;
  // two workgroups per CU; every slice costs one inverse transform and one partial result, so a slice
  // gets at least 4 iterations of work
  int64_t slices = std::max<int64_t>(1, (2 * (int64_t)cus + types - 1) / types);
  slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_items / (4 * nb)));
  int64_t ipw = (n_items + slices - 1) / slices;
  ipw = (ipw + nb - 1) / nb * nb;
  g->ipw = (int)ipw;
  g->slices = (int)((n_items + ipw - 1) / ipw);
  return 1;
}
}  // namespace

extern "C" {

int fc_wgrad1d_slices(const fc_desc* desc) {
  if (!desc) return 0;
  WgradGeom g;
  if (!wgrad_geometry(*desc, &g)) return 0;
  Twiddles tw;                                   // first use on this device: build the tables here, not in the launch
  if (get_twiddles(g.t, &tw) != FC_OK) return 0;
  return g.slices;
}

int fc_wgrad1d_db_supported(const fc_desc* desc) {
  if (!desc) return 0;
  WgradGeom g;
  return wgrad_geometry(*desc, &g) && !g.diag;
}

int fc_wgrad1d(const fc_desc* desc, const float* x, const float* dy, float* partial, int slices, void* hip_stream) {
  return fc_wgrad1d_db(desc, x, dy, partial, nullptr, 0, slices, hip_stream);
}

int fc_wgrad1d_db(const fc_desc* desc, const float* x, const float* dy, float* partial, float* db_partial,
                  long long slice_stride, int slices, void* hip_stream) {
  if (!desc || !x || !dy || !partial) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // a stale sticky error of an earlier, unrelated call (e.g. an invalidated capture) is not this call's
  WgradGeom g;
  if (!wgrad_geometry(*desc, &g)) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad1d does not cover this shape");
  if (db_partial && g.diag) return fail(FC_ERR_UNSUPPORTED, "the depthwise weight-gradient kernel has no bias-gradient output "
                                        "(ask fc_wgrad1d_db_supported first)");
  {
    const long long dense = (long long)desc->out_channels * (desc->in_channels / desc->groups) * desc->kernel[0];
    if (slice_stride == 0) slice_stride = dense;
    if (slice_stride < dense) return fail(FC_ERR_INVALID, "slice_stride %lld is smaller than one partial tensor (%lld floats)", slice_stride, dense);
  }
  if (slices != g.slices) return fail(FC_ERR_INVALID, "partial holds %d slices, the plan needs %d", slices, g.slices);
  Twiddles tw;
  int rc = find_twiddles(g.t, &tw);
  if (rc != FC_OK) return rc;
  const fc_desc& d = *desc;
  fc::WGradArgs a;
  a.x = x; a.dy = dy; a.part = partial; a.twA = tw.twA; a.twB = tw.twB;
  a.B = (int)d.batch; a.Cin = (int)d.in_channels; a.Cout = (int)d.out_channels;
  a.G = g.diag ? (int)(d.groups / 8) : (int)d.groups;
  a.Cig = g.Cig; a.Cog = g.Cog; a.L = (int)d.spatial[0]; a.pad = g.pad; a.pad_mode = d.padding_mode;
  a.Lout = g.Lout;
  a.stride = (int)d.stride[0]; a.Lext = (a.Lout - 1) * a.stride + 1;
  a.dil = (int)d.dilation[0]; a.V = g.V; a.ntiles = g.ntiles;
  a.n_items = g.n_items; a.items_per_slice = g.ipw; a.nob = g.nob; a.nib = g.nib;
  a.scale = 1.0f / (4.0f * (float)g.t->T);
  a.Krow = (int)d.kernel[0];
  a.part_stride = slice_stride;
  a.io = d.dtype;                                  // FC_F32 (0), FC_F16 or FC_BF16 (fft_engine.hpp IO_CODE_*)
  const int64_t grid = g.diag ? (int64_t)g.slices * (d.groups / 8) : (int64_t)g.slices * d.groups * g.nob * g.nib;
  if (grid > 0x7fffffff) return fail(FC_ERR_UNSUPPORTED, "grid too large");
  for (int j = 0; j < g.nseg; ++j) {
    a.tap0 = j * g.seg_taps;
    a.K = std::min(g.seg_taps, (int)d.kernel[0] - a.tap0);
    a.pos_shift = a.tap0 * (int)d.dilation[0];
    a.dbpart = j == 0 ? db_partial : nullptr;      // every segment sees all of dY: the bias gradient comes from the first
    if (g.diag) FC_HIP(g.t->wgrad1d_diag(a, (int)grid, (hipStream_t)hip_stream));
    else FC_HIP(g.t->wgrad1d(a, (int)grid, (hipStream_t)hip_stream));
  }
  return FC_OK;
}

}  // extern "C"
